// kr_device.hpp -- device-side Kerr null-geodesic arithmetic for gfx950 (MI355X).
//
// One ray per work-item; the whole ray state lives in VGPRs.  Everything here is a pure
// __device__ function of registers: no memory traffic, no LDS, no cross-lane ops.  The per-step
// semantics follow the reference propagators (file:line cited per function, paths relative to the
// reference tree); arithmetic is written with the reference's association so that, built with
// -ffp-contract=off, a step differs from the CPU result only through the device libm (sin, cos,
// pow: <= 1-2 ulp vs glibc), never through re-ordering.
//
// Layout: kr_arith.hpp (scalar building blocks) -> this file (per-launch constants, per-lane state, the strict derivative evaluation, the
// fixed-step integrators, the stop surfaces, the epilogue) -> kr_fast.hpp (the fast-arithmetic evaluation, included below) -> kr_rk45.hpp
// (the adaptive integrator, included at the end).
//
// T = double is the product precision; T = float mirrors the reference's second instantiation
// (raytracer.cpp:1896-1897).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/kr_trace.h"
#include "kr_arith.hpp"

// The wave-uniform guards of the fast Euler / RK4 step with a theta-limit stop (step_fixed): each puts work that nearly every step of nearly every ray
// does for nothing behind ONE ballot, and is exact -- a wave with a lane that fails it runs the code as it was, a lane that passes provably gets what
// that code gives.  KR_UNIFORM_GUARDS: which of them the library is built with (a sum of UniformGuards; 0: the step as it was -- A/B builds).
// KR_GUARD_STATS=1 (diagnostic builds only, like KR_OCC_STATS): how many wave-steps each guard lets through, printed by trace_wait.
#ifndef KR_UNIFORM_GUARDS
#define KR_UNIFORM_GUARDS 3
#endif
#ifndef KR_GUARD_STATS
#define KR_GUARD_STATS 0
#endif

namespace kr {

enum UniformGuards { kGuardQuiet = 1, kGuardCap = 2 };
// KR_GUARD_STATS: {wave-steps at the site, of them all lanes pass} for the quiet guard [0, 1], "N >= 0 and R > 0" in k1 [2, 3] (counted only) and the
// cap guard [4, 5]; {wave-steps, all lanes in sine band 0, all in band 1} [6..8] (counted only)
constexpr int kGuardStatWords = 9;

// ---- per-launch constants (kernarg) -----------------------------------------------------------
template <typename T> struct TraceConsts {
    T a, horizon, rlim, thetalim;
    // theta_in_lo = max(theta_lo, 0), theta_in_hi = min(theta_hi, pi): the loop condition's theta interval (below) cut to [0, pi], where reflect_poles
    // leaves an angle alone -- the quiet-step guard of the fast Euler / RK4 step (step_fixed).  A NaN thetalim: (0, -inf), empty like (theta_lo, theta_hi).
    // (They stand where maxtstep_rlim and max_phistep stood, which no kernel read -- tstep_rlim_eff and phistep_eff are what the step compares against --
    // so every other member, and every kernel argument after the struct, keeps its offset.)
    T precision, theta_precision, max_tstep, theta_in_lo, theta_in_hi, tol;
    T sp0, sp1, sp2, sp3;   // stop_params
    T inv_precision, inv_theta_precision;   // RN(1/precision), RN(1/theta_precision): fast path, and div_by_uniform on the strict one
    bool inv_ok;                            // both divisors qualify for div_by_uniform
    bool rk45_extrapolate;                  // RK45: creeping captured rays are extrapolated to the step limit (default)
    bool equator_inside;                    // theta_in_lo < pi/2 < theta_in_hi: a step that ends inside the interval may still have crossed the equator
    int32_t steplim;
    int32_t stop_kind;
    // The optional clauses of the step heuristic ("if (max_tstep > 0 && r < maxtstep_rlim) ...", "if (max_phistep > 0) ...", "if (rlim > 0 && ...)",
    // "if (thetalim > 0 && ...)", raytracer.cpp:855-871) with the launch-uniform half folded into the constant the per-ray half compares against:
    // a disabled clause gets the value that makes its own comparison false for every ray (r < -inf; step > |inf / phidot|; x > +inf).  Same
    // decisions on every ray, and no uniform lane masks for the compiler to carry (and spill) through the step loop.
    T tstep_rlim_eff;       // max_tstep > 0 ? maxtstep_rlim : -inf
    // fast path: the words of max_tstep, and the high word of "no cap" -- a number >= 8.9e307 that shares max_tstep's low word (step_fixed)
    uint32_t tstep_lo, tstep_on_hi, tstep_off_hi;
    T phistep_eff;          // max_phistep > 0 ? max_phistep : +inf
    // ("rlim > 0 && r + rdot step > rlim" needs no constant of its own: with rlim <= 0 the loop condition r < rlim admits no step at all.
    // Likewise "thetalim > 0 && theta + thetadot step > thetalim" compares against theta_hi below: +inf unless thetalim > 0.)
    // loop condition of the theta-limit overloads, (tl > 0 && theta < tl) || (tl < 0 && theta > |tl|) || tl == 0  (:799), as theta_lo < theta < theta_hi:
    // tl > 0: (-inf, tl);  tl < 0: (|tl|, +inf);  tl == 0: (-inf, +inf);  NaN: empty (theta_hi = -inf)
    T theta_lo, theta_hi;
};

// the members that follow from thetalim alone (make_consts on the host; the probe kernel of kr_post.hip on the device)
template <typename T>
__host__ __device__ inline void set_theta_limits(TraceConsts<T>& c)
{
    const T inf = (T) __builtin_inf();
    c.theta_lo = c.thetalim < 0 ? -c.thetalim : -inf;
    c.theta_hi = c.thetalim > 0 ? c.thetalim : (c.thetalim <= 0 ? inf : -inf);
    c.theta_in_lo = c.theta_lo > 0 ? c.theta_lo : T(0);
    c.theta_in_hi = c.theta_hi < T(kPi) ? c.theta_hi : T(kPi);
    c.equator_inside = c.theta_in_lo < T(kPi2) && T(kPi2) < c.theta_in_hi;
}

// ---- per-lane ray state ---------------------------------------------------------------------
template <typename T> struct Lane {
    T t, r, theta, phi;
    T pt, pr, ptheta, pphi;
    T k, h, Q;
    int32_t rdot_sign, thetadot_sign, rdot_flips, eq_cross;
    int32_t steps;          // steps taken in THIS call (the reference's local `steps`)
    int32_t status;
    int32_t steps0;         // rays[i].steps on entry (>= 0 for a traced ray); its SIGN BIT is this call's "always evaluate the NEG_ENERGY flag" mark (energy_guard)
    bool r_was_positive, theta_was_positive;   // per-call locals, raytracer.cpp:767-768
    // RK45 only
    T step;                 // running step size
    T theta_eq_prev;
    T theta_prev;
    bool in_retry;          // a trial step was rejected: next iteration retries with the same k1
    int32_t creep_m;        // theta advanced by exactly this many ulps in the last creeping outer step (0: none) ...
    int32_t creep_run;      // ... and in this many consecutive outer steps before it
    bool creep_mode;        // the rest of the ray is replayed step by step from k1 alone (step_rk45)
    T creep_dt, creep_dphi; // its t and phi increments per step
    // RK45, strict arithmetic: what the accepted trial's last stage (k7) already knows about the point the next step's k1 is taken at
    bool fsal_valid;
    T f_sin2theta, f_rhosq, f_delta, f_pt, f_thetadotsq, f_abs_ptheta;
#if KR_GUARD_STATS
    unsigned long long guard_stats[kGuardStatWords];      // this lane's tallies (trace_body zeroes and sums them): a wave-step is counted by its first active lane
#endif
};

#if KR_GUARD_STATS
// word: the site's "wave-steps" word; pass0 / pass1: this lane passes (the site's first / second "all lanes" word; the second only where the site has one)
template <typename T> KR_DEV void guard_count(Lane<T>& s, int word, bool pass0, bool pass1 = false, bool two = false)
{
    const unsigned long long active = __builtin_amdgcn_ballot_w64(true);
    const bool all0 = __builtin_amdgcn_ballot_w64(!pass0) == 0, all1 = __builtin_amdgcn_ballot_w64(!pass1) == 0;
    if ((int) (threadIdx.x & 63) == __ffsll((long long) active) - 1) {
        ++s.guard_stats[word];
        if (all0) ++s.guard_stats[word + 1];
        if (two && all1) ++s.guard_stats[word + 2];
    }
}
#define KR_GUARD_COUNT(...) guard_count(__VA_ARGS__)
#else
#define KR_GUARD_COUNT(...) ((void) 0)
#endif

// The NEG_ENERGY flag, (1 - 2r/rho^2) tdot + (2 a r sin^2/rho^2) phidot < 0 (raytracer.cpp:264-273 / :874-887 / :1403-1410), is the conserved energy k
// evaluated from tdot and phidot.  Its two terms are <= ~(r^2 + a^2)^2 (k + |h| / r) / (rho^2 Delta) in size, so their rounding errors (1e-16 of the terms)
// stay far below k -- and the sum cannot come out negative, in the reference or here -- as long as the ray is not within 1e-6 of the horizon, k > 0 and
// |h| <= 1e6 k.  The per-ray half of that (k, h: constants of the ray) is decided ONCE, when a lane takes the ray, and kept in the sign bit of steps0;
// the per-step test is then "r - r_h > 1e-6 and the mark is clear" -- two compares, as before the |h| clause existed.
template <typename T> KR_DEV void energy_guard_set(Lane<T>& s)
{
    if (!(s.k > T(0)) || !(kr_abs(s.h) <= T(1e6) * s.k)) s.steps0 |= (int32_t) 0x80000000;       // (NaN k or h: marked)
}
template <typename T> KR_DEV bool energy_flag_needed(const Lane<T>& s, T r_minus_horizon) { return !(r_minus_horizon > T(1e-6)) || s.steps0 < 0; }
template <typename T> KR_DEV int32_t steps_on_entry(const Lane<T>& s) { return s.steps0 & 0x7fffffff; }

// The five denominators of one derivative evaluation (kerr.h:308-334: rho^2 Delta, sin^2 x that, sin, rho^4, rho^2) are products of one another, so
// in double precision three reciprocals are taken from the hardware -- of rho^2 Delta, sin and rho^2 -- and the other two are put together from them
// and polished (lean_recip_from): two quarter-rate instructions less per evaluation on the strict path, whose quotients stay the correctly rounded
// ones (tests/test_gpu_primitives.py; every ray record of 2e6-ray Euler / RK4 and 1e6-ray RK45 traces unchanged, profiles/r04_ab_experiments.txt).
// Every quotient is formed against the denominator AS THE REFERENCE ROUNDS IT (rho^2 x rho^2; sin^2 x (rho^2 Delta) or (sin^2 rho^2) Delta).
// (1 / rho^2 is NOT taken from 1 / (rho^2 Delta): exactly on the horizon, Delta = 0, the reference's thetadot^2 is still finite.)
template <typename T> struct StageRecips;
template <> struct StageRecips<double> {
    double rhosq_delta, sin_theta, sin2_rhosq_delta, rho4, rhosq;
    double y_rhosq_delta, y_sin, y_sin2_rhosq_delta, y_rho4, y_rhosq;
    KR_DEV StageRecips(double rhosq_delta_, double sin_theta_, double sin2_rhosq_delta_, double rhosq_, double delta)
        : rhosq_delta(rhosq_delta_), sin_theta(sin_theta_), sin2_rhosq_delta(sin2_rhosq_delta_), rho4(rhosq_ * rhosq_), rhosq(rhosq_)
    {
        y_rhosq_delta = lean_recip(rhosq_delta);
        y_sin = lean_recip(sin_theta);
        y_rhosq = lean_recip(rhosq);
        y_sin2_rhosq_delta = lean_recip_from(sin2_rhosq_delta, y_sin * (y_sin * y_rhosq_delta));      // (in this order: (1 / sin)^2 alone overflows for theta < 1e-154, long before the quotient does)
        y_rho4 = lean_recip_from(rho4, y_rhosq * y_rhosq);
    }
    KR_DEV double over_rhosq_delta(double x) const { return lean_div_y(x, rhosq_delta, y_rhosq_delta); }
    KR_DEV double over_sin(double x) const { return lean_div_y(x, sin_theta, y_sin); }
    KR_DEV double over_sin2_rhosq_delta(double x) const { return lean_div_y(x, sin2_rhosq_delta, y_sin2_rhosq_delta); }
    KR_DEV double over_rho4(double x) const { return lean_div_y(x, rho4, y_rho4); }
    KR_DEV double over_rhosq(double x) const { return lean_div_y(x, rhosq, y_rhosq); }
};
template <> struct StageRecips<float> {
    float rhosq_delta, sin_theta, sin2_rhosq_delta, rho4, rhosq, y_rhosq;
    KR_DEV StageRecips(float rhosq_delta_, float sin_theta_, float sin2_rhosq_delta_, float rhosq_, float)
        : rhosq_delta(rhosq_delta_), sin_theta(sin_theta_), sin2_rhosq_delta(sin2_rhosq_delta_), rho4(rhosq_ * rhosq_), rhosq(rhosq_), y_rhosq(0.0f) {}
    KR_DEV float over_rhosq_delta(float x) const { return x / rhosq_delta; }
    KR_DEV float over_sin(float x) const { return x / sin_theta; }
    KR_DEV float over_sin2_rhosq_delta(float x) const { return x / sin2_rhosq_delta; }
    KR_DEV float over_rho4(float x) const { return x / rho4; }
    KR_DEV float over_rhosq(float x) const { return x / rhosq; }
};

// momentum_from_consts, src/include/kerr.h:300-335
// SMALL_ANGLE (double): the caller vouches for |theta| < KR_SMALL_ANGLE_LIMIT (step_fixed's side-launch stages): kr_sincos_f64's small-angle branch
// without its test.
template <typename T, bool LONE = false, bool SMALL_ANGLE = false>
KR_DEV void momentum_impl(T& pt, T& pr, T& ptheta, T& pphi, T k, T h, T Q, int rdot_sign, int thetadot_sign, T r, T theta, T a, Lane<T>* keep = nullptr)
{
    T sin_theta, cos_theta;
    if constexpr (SMALL_ANGLE && sizeof(T) == 8) kr_sincos_small_f64(theta, sin_theta, cos_theta);
    else kr_sincos<LONE>(theta, sin_theta, cos_theta);
    const T sin2theta = sin_theta * sin_theta;
    const T rhosq = r * r + (a * cos_theta) * (a * cos_theta);
    const T delta = r * r - 2 * r + a * a;
    const T rhosq_delta = rhosq * delta;
    const StageRecips<T> y(rhosq_delta, sin_theta, sin2theta * rhosq_delta, rhosq, delta);
    pt = (rhosq * (r * r + a * a) + 2 * a * a * r * sin2theta) * k - 2 * a * r * h;
    pt = y.over_rhosq_delta(pt);

    pphi = 2 * a * r * sin2theta * k + (rhosq - 2 * r) * h;
    pphi = y.over_sin2_rhosq_delta(pphi);

    const T hcs = y.over_sin(h * cos_theta);
    T thetadotsq = Q + (k * a * cos_theta + hcs) * (k * a * cos_theta - hcs);
    thetadotsq = y.over_rho4(thetadotsq);
    const T abs_ptheta = sq(kr_abs(thetadotsq));
    ptheta = abs_ptheta * thetadot_sign;
    if (keep) {      // (see k1_from_last_stage)
        keep->f_sin2theta = sin2theta; keep->f_rhosq = rhosq; keep->f_delta = delta; keep->f_pt = pt; keep->f_thetadotsq = thetadotsq; keep->f_abs_ptheta = abs_ptheta;
    }

    T rdotsq = k * pt - h * pphi - rhosq * ptheta * ptheta;
    rdotsq = y.over_rhosq(rdotsq * delta);
    pr = sq(kr_abs(rdotsq)) * rdot_sign;
}

template <typename T>
KR_DEV void momentum(T& pt, T& pr, T& ptheta, T& pphi, T k, T h, T Q, int rdot_sign, int thetadot_sign, T r, T theta, T a)
{
    momentum_impl<T>(pt, pr, ptheta, pphi, k, h, Q, rdot_sign, thetadot_sign, r, theta, a);
}

// k1 at the current position with turning-point logic; identical in all five reference propagators
// (raytracer.cpp:177-222, :805-849, :1086-1130, :1370-1398, :1680-1708).  RK45_ASSOC selects the RK45
// bodies' association of the phidot denominator ((sin2theta*rhosq)*delta, :1375 vs :818).
// Returns true when the reference would `continue` (theta turning point: sign flipped, nothing moves).
template <typename T, bool RK45_ASSOC, bool LONE = false>
KR_DEV bool k1_with_flips(Lane<T>& s, T a, T& rhosq_o, T& sin2theta_o, T* y_rhosq_o = nullptr)
{
    const T r = s.r, theta = s.theta, k = s.k, h = s.h;
    T sin_theta, cos_theta;
    kr_sincos<LONE>(theta, sin_theta, cos_theta);
    const T sin2theta = sin_theta * sin_theta;
    const T rhosq = r * r + (a * cos_theta) * (a * cos_theta);
    const T delta = r * r - 2 * r + a * a;
    const T rhosq_delta = rhosq * delta;
    const StageRecips<T> y(rhosq_delta, sin_theta, RK45_ASSOC ? sin2theta * rhosq * delta : sin2theta * rhosq_delta, rhosq, delta);
    s.pt = y.over_rhosq_delta((rhosq * (r * r + a * a) + 2 * a * a * r * sin2theta) * k - 2 * a * r * h);
    s.pphi = y.over_sin2_rhosq_delta(2 * a * r * sin2theta * k + (rhosq - 2 * r) * h);

    const T hcs = y.over_sin(h * cos_theta);
    T thetadotsq = s.Q + (k * a * cos_theta + hcs) * (k * a * cos_theta - hcs);
    thetadotsq = y.over_rho4(thetadotsq);

    if (thetadotsq < 0 && s.theta_was_positive) {
        s.thetadot_sign = -s.thetadot_sign;
        s.theta_was_positive = false;
        return true;
    }
    if (thetadotsq >= 0) s.theta_was_positive = true;

    s.ptheta = sq(kr_abs(thetadotsq)) * s.thetadot_sign;

    T rdotsq = k * s.pt - h * s.pphi - rhosq * s.ptheta * s.ptheta;
    const T y_rhosq = y.y_rhosq;                // (the caller's two flag quotients over rho^2 reuse it: step_fixed)
    rdotsq = y.over_rhosq(rdotsq * delta);
    if constexpr (LONE) {
        // (the same bookkeeping as selects: the if / else costs a wave that owns its SIMD a taken branch around a one-instruction else arm on every step)
        const bool flip = rdotsq <= 0 && s.r_was_positive;
        s.rdot_sign = flip ? -s.rdot_sign : s.rdot_sign;
        s.rdot_flips += flip ? 1 : 0;
        s.r_was_positive = !flip && (s.r_was_positive || rdotsq > 0);
    } else if (rdotsq <= 0 && s.r_was_positive) {
        s.rdot_sign = -s.rdot_sign;
        s.r_was_positive = false;
        s.rdot_flips++;
    } else if (rdotsq > 0) {
        s.r_was_positive = true;
    }
    s.pr = sq(kr_abs(rdotsq)) * s.rdot_sign;

    rhosq_o = rhosq;
    sin2theta_o = sin2theta;
    if (y_rhosq_o) *y_rhosq_o = y_rhosq;
    return false;
}

// RK45: the k1 of a step that follows an ACCEPTED trial is taken at the point that trial's last stage (k7) was evaluated at, and most
// of it is the same arithmetic on the same operands: sin^2, rho^2, Delta, tdot, thetadot^2 and |thetadot| come out bit for bit as k7
// had them (momentum_impl above and k1_impl evaluate identical expressions; the reference recomputes them, :1370-1398).  What differs
// is phidot -- the RK45 bodies associate its denominator as (sin^2 rho^2) Delta, kerr.h as sin^2 (rho^2 Delta) -- and rdot^2, which
// depends on it; those, the turning-point logic and the signs are done here as k1_impl does them.  ~70-115 of a trial step's ~1400
// instructions, on every accepted step; exact.  (Strict arithmetic, double precision.)
template <typename T>
KR_DEV bool k1_from_last_stage(Lane<T>& s, T a, T& rhosq_o, T& sin2theta_o, T* y_rhosq_o = nullptr)
{
    const T r = s.r, k = s.k, h = s.h;
    const T sin2theta = s.f_sin2theta, rhosq = s.f_rhosq, delta = s.f_delta;
    s.pt = s.f_pt;
    s.pphi = dv(2 * a * r * sin2theta * k + (rhosq - 2 * r) * h, sin2theta * rhosq * delta);
    const T thetadotsq = s.f_thetadotsq;
    if (thetadotsq < 0 && s.theta_was_positive) {
        s.thetadot_sign = -s.thetadot_sign;
        s.theta_was_positive = false;
        return true;
    }
    if (thetadotsq >= 0) s.theta_was_positive = true;
    s.ptheta = s.f_abs_ptheta * s.thetadot_sign;
    T rdotsq = k * s.pt - h * s.pphi - rhosq * s.ptheta * s.ptheta;
    const T y_rhosq = dv_recip(rhosq);                 // (shared with the caller's two flag quotients over rho^2, as in k1_with_flips)
    rdotsq = dv_y(rdotsq * delta, rhosq, y_rhosq);
    if (rdotsq <= 0 && s.r_was_positive) {
        s.rdot_sign = -s.rdot_sign;
        s.r_was_positive = false;
        s.rdot_flips++;
    } else if (rdotsq > 0) {
        s.r_was_positive = true;
    }
    s.pr = sq(kr_abs(rdotsq)) * s.rdot_sign;
    rhosq_o = rhosq;
    sin2theta_o = sin2theta;
    if (y_rhosq_o) *y_rhosq_o = y_rhosq;
    return false;
}

}  // namespace kr

#include "kr_fast.hpp"

namespace kr {

// one derivative evaluation on either path
template <typename T, bool FAST, bool LONE = false>
KR_DEV void eval(T& pt, T& pr, T& ptheta, T& pphi, const Lane<T>& s, T r, T theta, T a)
{
    if constexpr (FAST) momentum_fast(pt, pr, ptheta, pphi, s.k, s.h, s.Q, s.rdot_sign, s.thetadot_sign, r, theta, a);
    else momentum_impl<T, LONE>(pt, pr, ptheta, pphi, s.k, s.h, s.Q, s.rdot_sign, s.thetadot_sign, r, theta, a);
}

// loop condition of the theta-limit overloads (raytracer.cpp:172, :799, :1362-1364) or of the
// RayDestination overloads (:1080, :1674)
template <typename T, bool USE_DEST>
KR_DEV bool loop_cond(const Lane<T>& s, const TraceConsts<T>& c)
{
    bool ok = s.r < c.rlim && s.steps < c.steplim;
    if (!USE_DEST) {
        ok = ok && s.theta < c.theta_hi && s.theta > c.theta_lo;        // (TraceConsts::theta_lo / theta_hi)
    }
    return ok;
}

// The quiet-step guard of the fast theta-limit step (step_fixed has the argument): true only for a lane that every test at the end of the step answers
// with "no" -- no pole reflection, no horizon, the loop condition holds.  A NaN fails it.
// (theta_in_lo, theta_in_hi: TraceConsts' pair, from wherever the instance keeps it.  "&": five compares and their scalar ands, no short-circuit branches.)
template <typename T>
KR_DEV bool quiet_step(const Lane<T>& s, const TraceConsts<T>& c, T theta_in_lo, T theta_in_hi)
{
    return (s.r > c.horizon) & (s.r < c.rlim) & (s.theta > theta_in_lo) & (s.theta < theta_in_hi) & (s.steps < c.steplim);
}

// KR_STOP_THICKDISC (include/kr_trace.h has the rule, one IEEE operation per line): the point (r, theta) against the body |z| <= H(rho) over
// r_in <= rho <= r_out.  False: out of range, nothing else is set.  |r| < r_in implies |rho| = |RN(r sin)| <= |r| < r_in (|sin| <= 1, rounding is
// monotone), which is out of range whatever theta is: that test comes before any trigonometry -- it is the answer for every ray inside r_in,
// the captured ones above all.  The sine and cosine are evaluated here: the strict step keeps sin^2 of the new point, not the pair.
template <typename T> struct ThickDiscPoint { T sn, cs, rho, z, H, root; };      // root = sqrt(r_in / rho)
template <typename T>
KR_DEV bool thick_disc_point(const TraceConsts<T>& c, T r, T theta, ThickDiscPoint<T>& p)
{
    const T r_in = c.sp0, r_out = c.sp1, slope = c.sp2, scale = c.sp3;
    if (kr_abs(r) < r_in) return false;
    kr_sincos(theta, p.sn, p.cs);
    p.rho = r * p.sn;
    p.z = r * p.cs;
    if (!((p.rho >= r_in) && !(r_out > 0 && p.rho > r_out))) return false;
    p.root = kr_sqrt(r_in / p.rho);
    p.H = slope * p.rho + scale * (1 - p.root);
    return true;
}

// RayDestination::reached(r, theta, phi, prev_theta): ray_destination.h:90-94 (FlatDisc, through the
// default crossing-aware overload :52-54), :130-142 (DiscWithISCO), :184-190 (FlatPlane); KR_STOP_THICKDISC: include/kr_trace.h
template <typename T>
KR_DEV bool dest_reached(const TraceConsts<T>& c, T r, T theta, T phi, T prev_theta)
{
    if (c.stop_kind == KR_STOP_THICKDISC) {
        ThickDiscPoint<T> p;
        if (!thick_disc_point(c, r, theta, p)) return false;
        return kr_abs(p.z) <= p.H || (prev_theta < T(kPi2) && theta >= T(kPi2)) || (prev_theta > T(kPi2) && theta <= T(kPi2));
    }
    if (c.stop_kind == KR_STOP_FLATDISC) {
        const T tl = c.sp0;
        if (tl > 0) return theta >= tl;
        if (tl < 0) return theta <= -tl;
        return false;
    }
    if (c.stop_kind == KR_STOP_DISC_ISCO) {
        const T r_isco = c.sp0, r_out = c.sp1, tl = c.sp2;
        if (r < r_isco) return false;
        if (r_out > 0 && r > r_out) return false;
        if (tl > 0) return (prev_theta < tl && theta >= tl) || (prev_theta > tl && theta <= tl);
        if (tl < 0) {
            const T m = -tl;
            return (prev_theta > m && theta <= m) || (prev_theta < m && theta >= m);
        }
        return false;
    }
    // KR_STOP_FLATPLANE
    const T incl = c.sp0, phi0 = c.sp1, z_s = c.sp2;
    const T proj = r * (kr_sin(theta) * kr_sin(incl) * kr_cos(phi - phi0) + kr_cos(theta) * kr_cos(incl));
    return proj <= -z_s;
}

// RayDestination::step_limit(): ray_destination.h:55-57 (base), :95-101, :143-151
template <typename T>
KR_DEV T dest_step_limit(const TraceConsts<T>& c, T r, T theta, T pr, T ptheta)
{
    T tl;
    if (c.stop_kind == KR_STOP_THICKDISC) {
        // linear extrapolation of f = |z| - H(rho) along the stage-1 momenta, floored at KR_MIN_STEP: on a curved surface the bare quotient shrinks
        // the clamped step geometrically and reached() never fires
        ThickDiscPoint<T> p;
        if (!thick_disc_point(c, r, theta, p)) return Lim<T>::max();
        const T sg = p.z < 0 ? T(-1) : T(1);
        const T f = sg * p.z - p.H;
        const T zdot = pr * p.cs - (r * p.sn) * ptheta;
        const T rhodot = p.sn * pr + (r * p.cs) * ptheta;
        const T Hp = c.sp2 + (c.sp3 * T(0.5) * p.root) / p.rho;
        const T fdot = sg * zdot - Hp * rhodot;
        if (f > 0 && fdot < 0) {
            const T q = f / -fdot;
            return q < T(KR_MIN_STEP) ? T(KR_MIN_STEP) : q;
        }
        return Lim<T>::max();
    }
    if (c.stop_kind == KR_STOP_FLATDISC) {
        tl = c.sp0;
    } else if (c.stop_kind == KR_STOP_DISC_ISCO) {
        if (r < c.sp0) return Lim<T>::max();
        if (c.sp1 > 0 && r > c.sp1) return Lim<T>::max();
        tl = c.sp2;
    } else {
        return Lim<T>::max();
    }
    if (tl > 0 && ptheta > 0 && theta < tl) return (tl - theta) / ptheta;
    if (tl < 0 && ptheta < 0 && theta > -tl) return (-tl - theta) / ptheta;
    return Lim<T>::max();
}

// polar reflection, raytracer.cpp:282-283 / :914-915 / :1498-1499
// sign_d (optional): the same sign as a double (FastRaySigns::thetadot), converted again where the integer flips
template <typename T, bool LONE = false>
KR_DEV void reflect_poles(T& theta, T& phi, int32_t& thetadot_sign, double* sign_d = nullptr)
{
    // a pole crossing is rare: one wave-uniform test, and the per-lane selects only in a wave that has one
    if constexpr (LONE) {
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(theta < T(0) || theta > T(kPi)) == 0, true)) return;     // (the usual path falls through)
    } else {
        if (__builtin_amdgcn_ballot_w64(theta < T(0) || theta > T(kPi)) == 0) return;
    }
    if (theta < T(0)) { theta = -theta; thetadot_sign = -thetadot_sign; if (sign_d) *sign_d = (double) thetadot_sign; phi += T(kPi); }
    if (theta > T(kPi)) { theta = T(2) * T(kPi) - theta; thetadot_sign = -thetadot_sign; if (sign_d) *sign_d = (double) thetadot_sign; phi += T(kPi); }
}

template <typename T>
KR_DEV bool crossed_equator(T before, T after)
{
    return ((double) before < kPi2 && (double) after >= kPi2) || ((double) before > kPi2 && (double) after <= kPi2);
}

// What a lane keeps of its ray's constants besides the lane state, from the moment it takes the ray (trace_body): the instances that carry them hold
// a FastRayConsts, every other instance an empty struct that nothing reads -- those kernels compile to what they were without it.
struct NoRayConsts {};
template <bool CARRIED> using RayConstsOf = std::conditional_t<CARRIED, FastRayConsts, NoRayConsts>;
// Likewise the signs as doubles and the launch's values in vector registers (kr_fast.hpp: FastRaySigns, FastLaunchRegs): the fast Euler / RK4 instances
// with a theta-limit stop.  Not the RayDestination ones: their RK4 kernels sit on the 168-register ceiling of three waves per SIMD with scratch in use.
template <bool CARRIED> using RaySignsOf = std::conditional_t<CARRIED, FastRaySigns, NoRayConsts>;
template <bool CARRIED> using LaunchRegsOf = std::conditional_t<CARRIED, FastLaunchRegs, NoRayConsts>;

// What a kernel instance carries through its step loop (trace_body's STEP_REGS, a sum of these): a group that is not carried reaches the step as the
// launch constant / literal it always was, and the step compiles to what it was without.
enum StepRegs { kStepSigns = 1, kStepTimeCap = 2, kStepNearLead = 4, kStepQuiet = 8, kStepRegsAll = 15 };

template <int WHAT> KR_DEV FastLaunchRegs fast_launch_regs(const TraceConsts<double>& c)
{
    FastLaunchRegs l;
    l.tstep_rlim = c.tstep_rlim_eff; l.near_s9 = 1.0 / 362880.0; l.near_c8 = 1.0 / 40320.0; l.tstep_lo = c.tstep_lo; l.tstep_on_hi = c.tstep_on_hi; l.tstep_off_hi = c.tstep_off_hi;
    // (opaque to the compiler from here on, as consts_into_vector_registers' are: values in vector registers, neither uniform nor constant)
    if constexpr ((WHAT & kStepTimeCap) != 0) asm("" : "+v"(l.tstep_rlim), "+v"(l.tstep_lo), "+v"(l.tstep_on_hi), "+v"(l.tstep_off_hi));
    if constexpr ((WHAT & kStepNearLead) != 0) asm("" : "+v"(l.near_s9), "+v"(l.near_c8));
    l.theta_in_lo = c.theta_in_lo; l.theta_in_hi = c.theta_in_hi; l.equator_inside = c.equator_inside;
    if constexpr ((WHAT & kStepQuiet) != 0) asm("" : "+v"(l.theta_in_lo), "+v"(l.theta_in_hi));
    return l;
}

// One iteration of the Euler (raytracer.cpp:172-313) or RK4 (:799-943, :1080-1229) loop body.
// Returns true when the ray has finished (break, or the loop condition no longer holds).
// rayc: the ray's constant terms, filled where the lane took the ray -- the fast path reads them, the others are called without.
// sg, lr (fast path, theta-limit stop): the ray's signs as doubles, kept in step with the integers here, and the launch's values in
// vector registers.  The step computes the same operations on the same operands with or without them.
template <typename T, bool RK4, bool USE_DEST, bool FAST, bool LONE = false>
KR_DEV bool step_fixed(Lane<T>& s, const TraceConsts<T>& c, const FastRayConsts* rayc = nullptr, FastRaySigns* sg = nullptr, const FastLaunchRegs* lr = nullptr)
{
    const T a = c.a;
    ++s.steps;
    // (the wave-uniform guards: the theta-limit instances only -- the RayDestination RK4 kernels sit on their register ceiling with scratch in use, and stay as they are)
    constexpr int kGuards = (FAST && !USE_DEST && sizeof(T) == 8) ? (KR_UNIFORM_GUARDS) : 0;

    T step;
    T pt1, pr1, ptheta1, pphi1;
    FastAux aux;
    if constexpr (FAST) {
        // (carrying sin / cos of the base point from step to step by angle addition was measured and rejected: it removes 7 of 406 vector instructions
        // per RK4 step but costs registers the stage code needs -- 63.2 ms against 62.7 at 1e7 rays, Euler 31.6 against 30.9; profiles/r03_ab_experiments.txt)
        if (k1_with_flips_fast(s, a, *rayc, aux, sg)) return !(s.steps < c.steplim);
        pt1 = s.pt; pr1 = s.pr; ptheta1 = s.ptheta; pphi1 = s.pphi;
        // The same heuristic (:855-871) with ONE quarter-rate instruction instead of four.  1 / |rdot| and 1 / |thetadot| come out of the
        // square roots that produced them (fast_sqrt); the time and azimuth caps, min(dt / |tdot|, dphi / |phidot|), share one reciprocal:
        // min(dt |phidot|, dphi |tdot|) / (|tdot| |phidot|).  A cap that is switched off is +inf in the numerator (TraceConsts), a NaN or 0 / 0
        // quotient leaves the step as it is (v_min ignores a NaN operand) -- as the reference's "step > x" does.
        const T inv_pr = aux.inv_abs_pr, inv_pth = aux.inv_abs_ptheta;          // magnitudes: every use below takes |.| anyway
        const T q_th = kr_abs(s.theta) * inv_pth;
        const T dr = s.r - c.horizon;
        step = (kr_abs(dr) * inv_pr) * c.inv_precision;
        if (step > q_th * c.inv_precision) step = q_th * c.inv_theta_precision;
        {
            // (|phidot| floored at 1e-300: with phidot == 0 exactly -- a = 0 and h = 0 -- the shared quotient below would be 0 x inf = NaN, v_min would
            // ignore it and the TIME cap would be dropped with it, where the reference's "step > |max_tstep / tdot|" applies it; floored, the
            // quotient is min(dt 1e-300, dphi |tdot|) / (|tdot| 1e-300) = dt / |tdot|)
            const T apt = kr_abs(pt1), aphi = abs_floor(pphi1);
            // the time cap applies inside maxtstep_rlim only: outside, "dt" is a huge number with max_tstep's LOW word (TraceConsts::tstep_off_hi),
            // so that the choice is one select on the high word instead of two on a 64-bit pair
            const bool capped = s.r < (lr ? lr->tstep_rlim : c.tstep_rlim_eff);
            const uint32_t dt_hi = capped ? (lr ? lr->tstep_on_hi : c.tstep_on_hi) : (lr ? lr->tstep_off_hi : c.tstep_off_hi);
            const T dt_eff = __builtin_bit_cast(double, ((unsigned long long) dt_hi << 32) | (lr ? lr->tstep_lo : c.tstep_lo));
            const T num = __builtin_fmin(dt_eff * aphi, c.phistep_eff * apt);
            const T m = apt * aphi;
            if constexpr ((kGuards & kGuardCap) != 0) {
                // The reciprocal chain only in a wave in which the cap can bind on some lane (cap_cannot_bind, kr_fast.hpp, has the proof).
                const bool free_lane = cap_cannot_bind(step, m, num);
                KR_GUARD_COUNT(s, 4, free_lane);
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(!free_lane) != 0, false)) {
                    asm volatile("");        // (as for the ERGO block below)
                    step = __builtin_fmin(step, num * fast_rcp_heur(m));
                }
            } else {
                step = __builtin_fmin(step, num * fast_rcp_heur(m));
            }
        }
        // "if (step < MIN_STEP) step = MIN_STEP" as v_max: differs from the comparison only when `step` is NaN, i.e. when r or rdot is -- and
        // then r is NaN after this step whatever its length
        if constexpr ((kGuards & kGuardCap) != 0) {
            // (the instruction itself: `step` may now reach this line straight from the select above, and the compiler then puts a canonicalising
            // v_max step, step in front of fmax.  That one only quiets a signalling NaN -- fp64 subnormals are kept -- and `step` is the result of an
            // arithmetic instruction on every path: the same bits without it.)
            asm("v_max_f64 %0, %1, %2" : "=v"(step) : "v"(step), "s"(T(KR_MIN_STEP)));
        } else {
            step = __builtin_fmax(step, T(KR_MIN_STEP));
        }
        // the two landing clips apply on a ray's LAST step only: one fused test each, the clip itself behind a wave-uniform branch (the empty
        // asm keeps the compiler from turning the branch back into unconditional arithmetic and selects).  The clipped step is the reference's
        // correctly rounded quotient: it decides whether theta + thetadot step lands ON the limit or an ulp short of it (= one more step).
        // With the heuristic's approximate reciprocal (2^-44) 23 of 1e6 Euler rays of a lamp post at a = 0 took that extra step
        // (profiles/r03_hybrid_sweep_euler.jsonl, tests/tool_gpu_euler_diff.py).
        {
            // (the fused sum is within an ulp of the reference's rounded product + rounded sum: ">=" lets every ray through that the reference's
            // own test, made inside, could clip)
            const bool near_r = __builtin_fma(pr1, step, s.r) >= c.rlim;
            if (__builtin_amdgcn_ballot_w64(near_r) != 0) {
                asm volatile("" ::: "memory");
                if (near_r && s.r + pr1 * step > c.rlim) step = kr_abs(lean_div(c.rlim - s.r, pr1));
            }
        }
        if (!USE_DEST) {
            const bool near_th = __builtin_fma(ptheta1, step, s.theta) >= c.theta_hi;
            if (__builtin_amdgcn_ballot_w64(near_th) != 0) {
                asm volatile("" ::: "memory");
                if (near_th && s.theta + ptheta1 * step > c.theta_hi) step = kr_abs(lean_div(c.theta_hi - s.theta, ptheta1));
            }
        }
        if (__builtin_amdgcn_ballot_w64(pt1 <= 0) != 0) {        // (inside the ergosphere only: one compare and a scalar branch instead of compare, or, select)
            asm volatile("");        // (cannot be speculated: without it the branch comes back as "or" and select on every step.  No memory clobber --
                                     // this block is on every step's way, and the merged kernels read their constants through a pointer)
            if (pt1 <= 0) s.status |= KR_STATUS_ERGO;
        }
        // (1 - 2r/rho^2) tdot + (2 a r sin^2/rho^2) phidot IS the conserved energy k (= -p_t): analytically it cannot turn negative, and
        // numerically only where its two terms (~ k / Delta) are 1e15 times k.  Away from the horizon, for k > 0, the test is skipped
        // (wave-uniform; a NaN k or r takes the evaluation, whose comparison is then false as in the reference).
        if (__builtin_amdgcn_ballot_w64(energy_flag_needed(s, dr)) != 0) {
            const T two_r_rho = 2 * s.r * aux.inv_rhosq;
            if ((1 - two_r_rho) * pt1 + (two_r_rho * a * aux.sin2theta) * pphi1 < 0) s.status |= KR_STATUS_NEG_ENERGY;
        }
    } else {
    T rhosq, sin2theta, y_rhosq;
    if (k1_with_flips<T, false, LONE>(s, a, rhosq, sin2theta, &y_rhosq)) return !(s.steps < c.steplim);   // r, theta unchanged
    pt1 = s.pt; pr1 = s.pr; ptheta1 = s.ptheta; pphi1 = s.pphi;

    // step-size heuristic (:224-243 / :855-871 / :1136-1151)
    step = div_const(kr_abs(dv(s.r - c.horizon, pr1)), c.precision, c.inv_precision, c.inv_ok);
    {
        const T q_th = kr_abs(dv(s.theta, ptheta1));
        if (step > div_const(q_th, c.precision, c.inv_precision, c.inv_ok)) step = div_const(q_th, c.theta_precision, c.inv_theta_precision, c.inv_ok);
    }
    if (s.r < c.tstep_rlim_eff) {                       // max_tstep > 0 && r < maxtstep_rlim  (TraceConsts)
        const T st = kr_abs(dv(c.max_tstep, pt1));
        if (step > st) step = st;
    }
    {                                                   // max_phistep > 0: otherwise the quotient is inf / NaN and the comparison false
        const T sp = kr_abs(dv(c.phistep_eff, pphi1));
        if (step > sp) step = sp;
    }
    if ((double) step < KR_MIN_STEP) step = T(KR_MIN_STEP);
    if (s.r + pr1 * step > c.rlim) step = kr_abs(dv(c.rlim - s.r, pr1));
    if (!USE_DEST) {
        if (s.theta + ptheta1 * step > c.theta_hi) step = kr_abs(dv(c.theta_hi - s.theta, ptheta1));
    }

    // flags (:264-273 / :874-887); neither ends the ray
    if (pt1 <= 0) s.status |= KR_STATUS_ERGO;
    // (1 - 2r/rho^2) tdot + (2 a r sin^2/rho^2) phidot is the conserved energy k (= -p_t) evaluated from tdot and phidot: its two terms are
    // bounded (energy_guard_set) so that with r - r_horizon > 1e-6 (Delta > 1e-9 for every a < 0.99999), k > 0 and |h| <= 1e6 k the sum cannot come out
    // negative, in the reference or here.  The flag is therefore only evaluated -- with the reference's operations -- by waves in which some ray is that
    // close to the horizon or carries the mark.
    const bool flag_somewhere = __builtin_amdgcn_ballot_w64(energy_flag_needed(s, s.r - c.horizon)) != 0;
    if (sizeof(T) == 4 || (LONE ? __builtin_expect(flag_somewhere, false) : flag_somewhere)) {       // (LONE: the evaluation out of line, the usual path falls through)
        if ((1 - dv_y(2 * s.r, rhosq, y_rhosq)) * pt1 + dv_y(2 * a * s.r * sin2theta, rhosq, y_rhosq) * pphi1 < 0) s.status |= KR_STATUS_NEG_ENERGY;
    }
    }

    const T theta_prev = s.theta;
    if (!RK4) {
        s.t += pt1 * step;
        s.r += pr1 * step;
        s.theta += ptheta1 * step;
        s.phi += pphi1 * step;
    } else {
        // k2..k4 use k1's signs and move only (r, theta)  (:889-905)
        // stage evaluation; the fast path gets sin/cos of the stage angle from those of the base point
        // Stages 2-4.  Fast path: sin/cos of the stage angles come from the base point's by angle addition, which is valid
        // while every stage stays within near_limit of it -- practically always.  The stages are therefore computed
        // optimistically, branch-free, and in the rare other case all three are redone with the full routine (one branch
        // per step instead of one per stage; nothing of `s` has been touched yet).
        double near_limit = 0;
        if constexpr (FAST) near_limit = sincos_near_limit(s.theta);
        T acc_t, acc_phi, acc_r, acc_theta, pt4, pr4, ptheta4, pphi4;
        auto stages = [&](auto near) -> bool {
            constexpr bool kNear = decltype(near)::value;
            bool within = true;
            auto stage = [&](T& pt, T& pr, T& ptheta, T& pphi, T r_stage, T dtheta) {
                if constexpr (FAST) {
                    double sn, cs;
                    if constexpr (kNear) {
                        within = within && (__builtin_fabs(dtheta) <= near_limit);
                        sincos_near(aux.sn, aux.cs, dtheta, sn, cs, lr);
                    } else {
                        kr_sincos_fast_f64(s.theta + dtheta, sn, cs);
                    }
                    if (sg) momentum_fast_sc(pt, pr, ptheta, pphi, s.k, s.h, s.Q, *rayc, sg->rdot, sg->thetadot, r_stage, sn, cs, a);
                    else momentum_fast_sc(pt, pr, ptheta, pphi, s.k, s.h, s.Q, *rayc, s.rdot_sign, s.thetadot_sign, r_stage, sn, cs, a);
                } else if constexpr (kNear) {
                    const T theta_stage = s.theta + dtheta;
                    within = within && (kr_abs(theta_stage) < T(KR_SMALL_ANGLE_LIMIT));
                    momentum_impl<T, LONE, true>(pt, pr, ptheta, pphi, s.k, s.h, s.Q, s.rdot_sign, s.thetadot_sign, r_stage, theta_stage, a);
                } else {
                    eval<T, false, LONE>(pt, pr, ptheta, pphi, s, r_stage, s.theta + dtheta, a);
                }
            };
            // x1 + 2 x2 as ONE fused multiply-add: 2 x2 is exact, so fma(2, x2, x1) rounds the same sum once -- the reference's bits (:908-912)
            // on either path, one instruction instead of two; the stage radius r + h pr is fused on the fast path only (the product rounds)
            const T half = step / 2;
            auto at = [&](T h, T v) -> T { if constexpr (FAST) return __builtin_fma(h, v, s.r); else return s.r + h * v; };
            T pt2, pr2, ptheta2, pphi2;
            stage(pt2, pr2, ptheta2, pphi2, at(half, pr1), half * ptheta1);
            acc_t = kr_fma2(pt2, pt1);
            acc_phi = kr_fma2(pphi2, pphi1);
            T pt3, pr3, ptheta3, pphi3;
            stage(pt3, pr3, ptheta3, pphi3, at(half, pr2), half * ptheta2);
            acc_t = kr_fma2(pt3, acc_t);
            acc_phi = kr_fma2(pphi3, acc_phi);
            acc_r = kr_fma2(pr3, kr_fma2(pr2, pr1));
            acc_theta = kr_fma2(ptheta3, kr_fma2(ptheta2, ptheta1));
            stage(pt4, pr4, ptheta4, pphi4, at(step, pr3), step * ptheta3);
            return within;
        };
        if constexpr (FAST) {
            if (!stages(std::true_type{})) stages(std::false_type{});
        } else if constexpr (LONE && sizeof(T) == 8) {
            // Strict path on a wave that owns its SIMD (polar-axis rays: the critical path of the pass).  Nothing covers such a wave's branch bubbles,
            // and kr_sincos_f64 costs two compare-dependent branches per stage to pick its small-angle formula.  While the base angle is small on
            // every lane the three stages take that formula unasked, record whether their angles were small too, and are redone with the full
            // routine if not: the same values, one branch instead of six.
            bool done = false;
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(kr_abs(s.theta) < T(KR_SMALL_ANGLE_LIMIT))) == 0, 1)) done = stages(std::true_type{});
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(!done) != 0, 0)) {
                if (!done) stages(std::false_type{});
            }
        } else {
            stages(std::false_type{});
        }
        // x += (step/6)(k1 + 2k2 + 2k3 + k4), summed left to right as in :908-912
        const T w = FAST ? step * T(1.0 / 6.0) : div_const(step, T(6), T(1.0 / 6.0), true);
        if constexpr (FAST) {
            s.t = __builtin_fma(w, acc_t + pt4, s.t);
            s.r = __builtin_fma(w, acc_r + pr4, s.r);
            s.theta = __builtin_fma(w, acc_theta + ptheta4, s.theta);
            s.phi = __builtin_fma(w, acc_phi + pphi4, s.phi);
        } else {
            s.t += w * (acc_t + pt4);
            s.r += w * (acc_r + pr4);
            s.theta += w * (acc_theta + ptheta4);
            s.phi += w * (acc_phi + pphi4);
        }
    }
    if constexpr ((kGuards & kGuardQuiet) != 0) {
        // The quiet step: a lane whose new point lies strictly inside (horizon, rlim) x (theta_in_lo, theta_in_hi) with steps to spare fails every test
        // below -- 0 <= theta_in_lo < theta < theta_in_hi <= pi: no pole reflection; r > horizon; the loop condition holds term by term (theta_in_hi <=
        // theta_hi, theta_in_lo >= theta_lo) -- and, where the interval does not contain pi/2, cannot have crossed the equator either: theta_prev passed
        // the loop condition before this step (at the claim or at the end of the step before; the early return above moves nothing).  With theta_in_hi <=
        // pi/2 that limit IS theta_hi, so theta_prev < pi/2 and theta < pi/2; with theta_in_lo >= pi/2 it IS theta_lo, so both are > pi/2: either
        // clause of crossed_equator wants one angle on each side, or the new one ON pi/2.  A NaN r or theta fails the guard.
        // One ballot of the lanes that are not quiet: empty in every wave-step in which no ray ends or is reflected, and then the block below is
        // skipped; else it runs as it is, for every lane (a quiet lane gets its "no" from each test).
        // Where the interval does contain pi/2 (launch-uniform: TraceConsts::equator_inside) the equator test stays in front of the guard -- four
        // compares and the guard's five instead of twelve; those launches count a crossing where they did.
        const bool equator_inside = lr ? lr->equator_inside : c.equator_inside;
        if (equator_inside) { if (crossed_equator(theta_prev, s.theta)) ++s.eq_cross; }
        const bool quiet = quiet_step(s, c, lr ? lr->theta_in_lo : c.theta_in_lo, lr ? lr->theta_in_hi : c.theta_in_hi);
        KR_GUARD_COUNT(s, 0, quiet);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!quiet) == 0, true)) return false;
        asm volatile("");
        if (!equator_inside) { if (crossed_equator(theta_prev, s.theta)) ++s.eq_cross; }
    } else {
        if (crossed_equator(theta_prev, s.theta)) ++s.eq_cross;
    }
    reflect_poles<T, LONE>(s.theta, s.phi, s.thetadot_sign, sg ? &sg->thetadot : nullptr);

    if (s.r <= c.horizon) { s.status |= KR_STATUS_HORIZON; return true; }
    if (USE_DEST) {
        if (dest_reached(c, s.r, s.theta, s.phi, theta_prev)) { s.status |= KR_STATUS_DEST; return true; }
    }
    return !loop_cond<T, USE_DEST>(s, c);
}

// ---- radial rays (strict double precision, Euler / RK4, theta-limit stop) ------------------------------------------------------------------------
// The polar numerator C = Q + (k a cos + h cos / sin)(k a cos - h cos / sin) of thetadot^2 = C / rho^4 depends on (Q, k, h, a, theta) only, not on r.
// A ray for which it rounds to exactly +-0 at its theta is RADIAL: thetadot^2 = +-0 / rho^4 = +-0, so no polar turning point is seen, thetadot =
// sqrt(+0) x sign = +-0, every stage angle is theta + x (+-0) = theta, the update adds +-0 -- the next step starts from the same theta and the same C,
// and by induction the whole ray is a one-dimensional problem in r.  (The beta = -pi column of a lamp-post PointSource, emitted with thetadot = 0: Q is
// built so that C cancels at the source's theta.  DESIGN.md 4.1.)  step_radial below is step_fixed's strict lone-wave path with everything that is a
// constant of such a ray taken from a block computed once, when a lane takes the ray, and everything that is an exact zero or a comparison that cannot
// hold left out; what remains has the same operands in the same association, hence the same bits.  The induction needs two things of every step that
// only the step itself can tell: a finite step length (x above) and, at the base point and at each stage, a rho^2 whose square and reciprocals neither
// overflow nor underflow (so that +-0 / rho^4 IS +-0 through the assembled reciprocal, and rho^2 x 0 x 0 is +0).  A step that does not meet them --
// r or rdot NaN or infinite, practically -- is taken back and done by step_fixed, as is the rest of that ray.
struct RadialRay {
    double sin2theta, acs2;     // sin^2 theta, (a cos theta)^2
    double y_sin;               // StageRecips::y_sin
    double ptheta0;             // +0 x thetadot_sign: the ray's thetadot, signed zero included
    bool general;               // not (or no longer) provably radial: this lane's ray takes step_fixed
};

// Is a ray with these constants radial at `theta`?  sn, cs, y_sin: kr_sincos of theta and lean_recip(sn), i.e. what k1_with_flips / momentum_impl
// hold at that angle; C is formed as they form it.  theta must also be a fixed point of reflect_poles and inside the theta limits (the loop condition
// and the epilogue then see a constant).  A NaN anywhere makes C NaN.
KR_DEV bool ray_is_radial(double k, double h, double Q, double r, double theta, double a, double theta_lo, double theta_hi, double sn, double cs, double y_sin)
{
    const double hcs = lean_div_y(h * cs, sn, y_sin);
    const double C = Q + (k * a * cs + hcs) * (k * a * cs - hcs);
    return C == 0.0 && kr_finite(k) && kr_finite(h) && kr_finite(Q) && kr_finite(r) && theta > 0.0 && theta < kPi && theta > theta_lo && theta < theta_hi;
}

// when a lane takes a ray: the block, and the decision itself -- made here again, from the state the lane holds, whatever put the ray on the list
KR_DEV void radial_claim(const Lane<double>& s, const TraceConsts<double>& c, RadialRay& q)
{
    double sn, cs;
    kr_sincos<true>(s.theta, sn, cs);
    q.sin2theta = sn * sn;
    q.acs2 = (c.a * cs) * (c.a * cs);
    q.y_sin = lean_recip(sn);
    q.ptheta0 = 0.0 * s.thetadot_sign;
    q.general = !ray_is_radial(s.k, s.h, s.Q, s.r, s.theta, c.a, c.theta_lo, c.theta_hi, sn, cs, q.y_sin);
}

KR_DEV bool radial_rhosq_in_range(double rhosq) { return rhosq > 0x1p-500 && rhosq < 0x1p500; }      // (NaN: false)

// tdot, phidot and rdot^2 at radius r: momentum_impl / k1_with_flips with the ray's constants, without the polar half
KR_DEV void radial_eval(double& pt, double& pphi, double& rdotsq, double& rhosq_o, double& y_rhosq_o, double k, double h, double r, double a, const RadialRay& q)
{
    const double sin2theta = q.sin2theta;
    const double rhosq = r * r + q.acs2;
    const double delta = r * r - 2 * r + a * a;
    const double rhosq_delta = rhosq * delta;
    const double sin2_rhosq_delta = sin2theta * rhosq_delta;
    const double y_rhosq_delta = lean_recip(rhosq_delta);
    const double y_rhosq = lean_recip(rhosq);
    const double y_sin2_rhosq_delta = lean_recip_from(sin2_rhosq_delta, q.y_sin * (q.y_sin * y_rhosq_delta));
    pt = lean_div_y((rhosq * (r * r + a * a) + 2 * a * a * r * sin2theta) * k - 2 * a * r * h, rhosq_delta, y_rhosq_delta);
    pphi = lean_div_y(2 * a * r * sin2theta * k + (rhosq - 2 * r) * h, sin2_rhosq_delta, y_sin2_rhosq_delta);
    rdotsq = lean_div_y((k * pt - h * pphi) * delta, rhosq, y_rhosq);       // (- rho^2 x 0 x 0 = - (+0): the identity, also on -0, inf and NaN)
    rhosq_o = rhosq;
    y_rhosq_o = y_rhosq;
}

// One iteration of the Euler / RK4 loop body for a radial ray on a wave that owns its SIMD.  Returns true when the ray has finished; sets q.general
// and leaves `s` as it found it when the step has to be done by step_fixed instead.
template <bool RK4>
KR_DEV bool step_radial(Lane<double>& s, RadialRay& q, const TraceConsts<double>& c)
{
    const double a = c.a, k = s.k, h = s.h;
    const double t0 = s.t, r0 = s.r, phi0 = s.phi, pt0 = s.pt, pr0 = s.pr, ptheta0 = s.ptheta, pphi0 = s.pphi;
    const int32_t rdot_sign0 = s.rdot_sign, rdot_flips0 = s.rdot_flips, status0 = s.status;
    const bool r_was_positive0 = s.r_was_positive;
    ++s.steps;

    double rhosq, y_rhosq, rdotsq;
    radial_eval(s.pt, s.pphi, rdotsq, rhosq, y_rhosq, k, h, r0, a, q);
    bool ok = radial_rhosq_in_range(rhosq);
    s.ptheta = q.ptheta0;
    {
        const bool flip = rdotsq <= 0 && s.r_was_positive;
        s.rdot_sign = flip ? -s.rdot_sign : s.rdot_sign;
        s.rdot_flips += flip ? 1 : 0;
        s.r_was_positive = !flip && (s.r_was_positive || rdotsq > 0);
    }
    s.pr = sq(kr_abs(rdotsq)) * s.rdot_sign;
    const double pt1 = s.pt, pr1 = s.pr, pphi1 = s.pphi;

    // step-size heuristic: the theta clause compares against |theta / +-0|, which is not a number, and the theta landing clip against theta itself
    double step = div_const(kr_abs(dv(r0 - c.horizon, pr1)), c.precision, c.inv_precision, c.inv_ok);
    if (r0 < c.tstep_rlim_eff) {
        const double st = kr_abs(dv(c.max_tstep, pt1));
        if (step > st) step = st;
    }
    {
        const double sp = kr_abs(dv(c.phistep_eff, pphi1));
        if (step > sp) step = sp;
    }
    if (step < KR_MIN_STEP) step = KR_MIN_STEP;
    if (r0 + pr1 * step > c.rlim) step = kr_abs(dv(c.rlim - r0, pr1));
    ok = ok && kr_finite(step);

    if (pt1 <= 0) s.status |= KR_STATUS_ERGO;
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(energy_flag_needed(s, r0 - c.horizon)) != 0, false)) {
        if ((1 - dv_y(2 * r0, rhosq, y_rhosq)) * pt1 + dv_y(2 * a * r0 * q.sin2theta, rhosq, y_rhosq) * pphi1 < 0) s.status |= KR_STATUS_NEG_ENERGY;
    }

    if (!RK4) {
        s.t += pt1 * step;
        s.r += pr1 * step;
        s.phi += pphi1 * step;
    } else {
        auto stage = [&](double& pt, double& pr, double& pphi, double r_stage) {
            double rdotsq_s, rhosq_s, y_s;
            radial_eval(pt, pphi, rdotsq_s, rhosq_s, y_s, k, h, r_stage, a, q);
            ok = ok && radial_rhosq_in_range(rhosq_s);
            pr = sq(kr_abs(rdotsq_s)) * s.rdot_sign;
        };
        const double half = step / 2;
        double pt2, pr2, pphi2, pt3, pr3, pphi3, pt4, pr4, pphi4;
        stage(pt2, pr2, pphi2, r0 + half * pr1);
        double acc_t = kr_fma2(pt2, pt1);
        double acc_phi = kr_fma2(pphi2, pphi1);
        stage(pt3, pr3, pphi3, r0 + half * pr2);
        acc_t = kr_fma2(pt3, acc_t);
        acc_phi = kr_fma2(pphi3, acc_phi);
        const double acc_r = kr_fma2(pr3, kr_fma2(pr2, pr1));
        stage(pt4, pr4, pphi4, r0 + step * pr3);
        const double w = div_const(step, 6.0, 1.0 / 6.0, true);
        s.t += w * (acc_t + pt4);
        s.r += w * (acc_r + pr4);
        s.phi += w * (acc_phi + pphi4);
    }

    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0, false)) {
        if (!ok) {
            s.t = t0; s.r = r0; s.phi = phi0; s.pt = pt0; s.pr = pr0; s.ptheta = ptheta0; s.pphi = pphi0;
            s.rdot_sign = rdot_sign0; s.rdot_flips = rdot_flips0; s.status = status0; s.r_was_positive = r_was_positive0;
            --s.steps;
            q.general = true;
            return false;
        }
    }
    if (s.r <= c.horizon) { s.status |= KR_STATUS_HORIZON; return true; }
    return !(s.r < c.rlim && s.steps < c.steplim);
}

// Epilogue shared by all propagators (raytracer.cpp:315-339, :945-969, :1231-1253, :1574-1597, :1872-1893):
// final status bits and the value of rays[i].steps to store.
template <typename T, bool USE_DEST>
KR_DEV int32_t finish_status(Lane<T>& s, const TraceConsts<T>& c)
{
    if (s.steps >= c.steplim)
        s.status |= KR_STATUS_STEPLIM;
    else if (s.r >= c.rlim)
        s.status |= KR_STATUS_RLIM;
    else if (!USE_DEST && (s.theta >= c.theta_hi || s.theta <= c.theta_lo))       // (tl > 0 && theta >= tl) || (tl < 0 && theta <= |tl|)
        s.status |= KR_STATUS_DEST;
    int32_t out_steps = steps_on_entry(s);
    if (s.steps > 0) out_steps += s.steps;
    if (s.status & KR_STATUS_STEPLIM) out_steps = -out_steps;
    return out_steps;
}

}  // namespace kr

#include "kr_rk45.hpp"
