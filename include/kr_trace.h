/*
 * kr_trace.h -- C ABI of libkrtrace.so, the MI355X (gfx950) Kerr null-geodesic hot path.
 *
 * The reference (wilkinsdr/raytrace_cpu) has no FFI/plugin layer: its boundary is the C++ class API
 * Raytracer<T> / PointSource<T> / ImagePlane<T> (src/raytracer/raytracer.h:85-198).  This header is
 * the thin C ABI that a replacement Raytracer<T> calls from inside those member functions; each entry
 * point below names the reference function (file:line, relative to the reference tree) it replaces.
 * The host-side mirror of the class API that does exactly that lives in raytrace_cpu_amd/host/.
 *
 * Conventions
 *   - plain C, no C++/torch types; all sizes are int64_t; all entry points return 0 on success and a
 *     negative KR_E* code on failure (kr_last_error() gives the message).  There is NO CPU fallback:
 *     without a usable HIP device every compute entry point returns KR_ENODEVICE.
 *   - "_dev" entry points take DEVICE pointers (hipMalloc / torch data_ptr) and a hipStream_t passed
 *     as void* (NULL = default stream); they enqueue work and return without synchronising unless a
 *     kr_stats* is requested (stats need the kernel's counters -> the call synchronises the stream).
 *   - entry points without "_dev" take HOST pointers, stage through private device buffers and return
 *     with the host arrays updated (the contract of Raytracer<T>::run_raytrace: results are in
 *     rays[] when it returns, raytracer.cpp:63-127).
 *   - kr_ray_f64 / kr_ray_f32 are layout-identical to Ray<double> / Ray<float>
 *     (raytracer.h:65-78; 144 B / 84 B), so `rays` can be handed over without conversion.
 */
#ifndef KR_TRACE_H_
#define KR_TRACE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KR_ABI_VERSION 16

/* error codes */
#define KR_OK          0
#define KR_EINVAL     -1   /* bad argument (NULL pointer, unknown integrator/stop kind, Euler+destination) */
#define KR_ENODEVICE  -2   /* no HIP device / HIP runtime unusable */
#define KR_EHIP       -3   /* a HIP call failed; see kr_last_error() */
#define KR_ENOMEM     -4

/* enum class Integrator { Euler, RK4, RK45 }  (raytracer.h:83) */
#define KR_EULER 0
#define KR_RK4   1
#define KR_RK45  2

/* stop surfaces: the theta-limit overloads (raytracer.cpp:129,755,1260) and the three concrete
 * RayDestination classes (ray_destination.h:86,116,173) as POD descriptors */
#define KR_STOP_THETA      0   /* theta_max field; stop_params unused */
#define KR_STOP_FLATDISC   1   /* stop_params = {theta_lim} */
#define KR_STOP_DISC_ISCO  2   /* stop_params = {r_isco, r_out, theta_lim} */
#define KR_STOP_FLATPLANE  3   /* stop_params = {incl, phi0, z_s} */
/* A disc of finite thickness, handed to the reference as a user-defined RayDestination (ray_destination.h:36-41): the body |z| <= H(rho) over
 * r_in <= rho <= r_out (r_out <= 0: open), rho = r sin(theta) the cylindrical radius, z = r cos(theta), H(rho) = slope rho + scale (1 - sqrt(r_in / rho)):
 * `slope` a constant opening ratio H / rho, `scale` the radiation-pressure Shakura-Sunyaev height (3 mdot / (2 eta)); both zero: the thin annulus.
 * Every line one IEEE operation in this association, sin / cos the strict trace's:
 *   in_range = (rho >= r_in) && !(r_out > 0 && rho > r_out)                                                          (a NaN: false)
 *   reached(r, theta, phi, prev) = in_range && (fabs(z) <= H || (prev < pi/2 && theta >= pi/2) || (prev > pi/2 && theta <= pi/2))
 *   reached(r, theta, phi)       = reached(r, theta, phi, theta)
 *   step_limit(r, theta, phi, pr, ptheta, pphi):  max unless in_range;  sg = z < 0 ? -1 : 1;  f = sg z - H;
 *     zdot = pr cos(theta) - (r sin(theta)) ptheta;  rhodot = sin(theta) pr + (r cos(theta)) ptheta;
 *     Hp = slope + (scale 0.5 sqrt(r_in / rho)) / rho;  fdot = sg zdot - Hp rhodot;
 *     (f > 0 && fdot < 0) ? max(f / -fdot, KR_MIN_STEP) : max
 * The equator clause keeps the thin limit and the thin inner parts of the body from being stepped over.  The floor at KR_MIN_STEP: on a curved
 * surface the bare linear extrapolation shrinks the clamped RK45 step geometrically and reached() never fires.
 * Known limits: RK4 has no landing clamp in the reference's RayDestination overload, so an RK4 ray stops up to one step INSIDE the body; rays that
 * enter through the vertical walls at r_in / r_out are not step-limited.
 * Refused (KR_EINVAL, the parameter named): r_in not positive, slope or scale negative, any of the four not finite. */
#define KR_STOP_THICKDISC  4   /* stop_params = {r_in, r_out, slope, scale} */

/* ray status bit flags (raytracer.h:58-63) + one extension */
#define KR_STATUS_DEST        (1 << 0)
#define KR_STATUS_HORIZON     (1 << 1)
#define KR_STATUS_RLIM        (1 << 2)
#define KR_STATUS_STEPLIM     (1 << 3)
#define KR_STATUS_ERGO        (1 << 4)
#define KR_STATUS_NEG_ENERGY  (1 << 5)
/* extension: the RK45 retry loop met a NaN error norm.  The reference never leaves that loop
 * (raytracer.cpp:1438-1541); the device path ends the ray and sets this bit instead. */
#define KR_STATUS_NAN         (1 << 6)

/* kr_params.flags */
#define KR_FLAG_FAST_MATH     (1 << 0)  /* f64 trace only: same formulas with shared reciprocals, Newton-refined rcp/rsq, FMA
                                           contraction and stage sin/cos by angle addition instead of IEEE division/sqrt and one
                                           sincos per evaluation (a few ulp per operation; ~1.6x faster).  Rays whose outcome is
                                           rounding-decided in the reference may end differently: prefer KR_FLAG_HYBRID.
                                           0 = strict: the reference's association with IEEE + - * / sqrt, no contraction.  (A strict
                                           launch of >= 2^18 rays also puts its ill-conditioned rays on a side launch -- see HYBRID --
                                           which changes where they run, never their bits; env KR_NO_ISOLATE=1 disables that.) */

#define KR_FLAG_HYBRID        (1 << 1)  /* f64 trace only: rays whose polar motion / axial angular momentum is a cancellation residue
                                           (their outcome in the reference is decided by rounding) and NaN rays are integrated on
                                           the strict path, in a side launch whose waves own their SIMDs; all other rays take the
                                           fast-math path.  Reproduces the reference on every ray class at ~1.4x the strict speed.
                                           Nothing in the call waits for the device: the number of flagged rays stays in device
                                           memory, where the launches read it.  The concurrent launch runs on a second, internal
                                           stream of its own priority level that belongs to `stream` (released by kr_stream_destroy /
                                           kr_shutdown).  Growing the per-ray selector of a pooled workspace allocates (hipMalloc,
                                           which does not synchronise); nothing is freed in the launch path.
                                           Ignored by the f32 entry points and when KR_FLAG_FAST_MATH is set. */
#define KR_FLAG_RK45_ITERATE_ALL (1 << 2) /* RK45: iterate creeping captured rays to the step limit one step at a time, as the reference does,
                                           instead of extrapolating them (kr_stats.rk45_extrapolated_steps) */
#define KR_FLAG_BLOCKS_PER_CU(n)      (((n) & 0xF) << 8)   /* resident 256-thread workgroups per CU for the trace kernel; 0 = default: 3 for the main
                                                              launch of a split trace, for n >= 2e7 and for fast-math with n >= 5e6, else 2 */
#define KR_FLAG_GET_BLOCKS_PER_CU(f)  (((f) >> 8) & 0xF)

/* defaults, raytracer.h:19-44 */
#define KR_PRECISION        100.0
#define KR_THETA_PRECISION  50.0
#define KR_MAXDT            1.0
#define KR_MAXDT_RLIM       100.0
#define KR_MAXDPHI          0.1
#define KR_STEPLIM          10000000
#define KR_RK45_STEPLIM     100000
#define KR_MIN_STEP         1e-3

typedef struct kr_ray_f64 {
    double t, r, theta, phi;
    double pt, pr, ptheta, pphi;
    double k, h, Q;
    double emit, redshift;
    int32_t steps, status, rdot_sign, thetadot_sign, rdot_flips, equatorial_crossings;
    double alpha, beta;
} kr_ray_f64;

typedef struct kr_ray_f32 {
    float t, r, theta, phi;
    float pt, pr, ptheta, pphi;
    float k, h, Q;
    float emit, redshift;
    int32_t steps, status, rdot_sign, thetadot_sign, rdot_flips, equatorial_crossings;
    float alpha, beta;
} kr_ray_f32;

/* Everything Raytracer<T>::run_raytrace reads besides rays[] (members raytracer.h:89-99 + call
 * arguments raytracer.h:112-122).  Doubles carry float values exactly for the f32 entry points. */
typedef struct kr_params {
    double spin;             /* as stored by Raytracer (ImagePlane has already negated it, imageplane.cpp:12) */
    double horizon;          /* kerr_horizon(spin) or set_boundary() value */
    double precision;        /* PRECISION */
    double theta_precision;  /* THETA_PRECISION */
    double max_tstep;        /* MAXDT */
    double maxtstep_rlim;    /* MAXDT_RLIM */
    double max_phistep;      /* MAXDPHI */
    double rk45_tol;         /* 1e-8 */
    double r_max;            /* rlim */
    double theta_max;        /* thetalim (KR_STOP_THETA only) */
    double stop_params[4];
    int32_t integrator;      /* KR_EULER / KR_RK4 / KR_RK45 */
    int32_t stop_kind;       /* KR_STOP_* */
    int32_t steplim;         /* <=0: STEPLIM for Euler/RK4, RK45_STEPLIM for RK45 (raytracer.cpp:80) */
    int32_t flags;           /* KR_FLAG_* */
} kr_params;

/* counters gathered by the trace kernel (what integrator_perf_test.cpp:82-93 derives on the host) */
typedef struct kr_stats {
    int64_t rays_total;      /* n */
    int64_t rays_traced;     /* rays that entered a propagate loop (steps >= 0 and < steplim on entry) */
    int64_t steps_total;     /* sum of per-call `steps` over traced rays (every ++steps, incl. theta-flip iterations) */
    int64_t rk45_attempts;   /* RK45: trial steps evaluated (accepted + rejected) */
    int64_t rk45_rejects;    /* RK45: trial steps rejected */
    double  kernel_ms;       /* trace kernel duration, HIP events on the launch stream */
    double  h2d_ms, d2h_ms;  /* host-buffer entry points only */
    int64_t rays_strict_side;       /* rays classified ill-conditioned and traced by the strict side launch (KR_FLAG_HYBRID, and
                                       strict launches of >= 2^18 rays); 0 when the trace was a single launch */
    int64_t rk45_stationary_steps;  /* RK45: steps (included in steps_total and rk45_attempts) that were replayed as bare t/phi
                                       additions after a captured ray reached an exact fp64 fixed point in (r, theta, step);
                                       bit-identical to iterating them (kr_device.hpp::step_rk45) */
    int64_t rk45_extrapolated_steps; /* RK45: steps (included in steps_total and rk45_attempts) of captured rays whose r was stationary
                                       and whose theta advanced by a constant number of ulps per step: extrapolated to the step
                                       limit (r, theta, every integer output exact; t, phi, momenta to ~1e-11) */
    double  strict_side_ms;         /* split traces: duration of the strict side launch (caller's stream) ... */
    double  main_ms;                /* ... and of the main launch beside it (internal stream); kernel_ms spans both.  0 otherwise */
    int64_t longest_ray_steps;      /* most steps one ray took in this call: a ray is one sequential chain on a wave, so the launch that
                                       carries it lasts at least this many wave steps whatever else the GPU does (DESIGN.md "Known limit") */
    int64_t longest_ray_steps_strict_side; /* the same over the rays of the strict side launch of a split trace (0 otherwise):
                                       strict_side_ms / this = that launch's time per step on a wave of its own */
    int64_t steps_strict_side;      /* steps_total of the strict side launch alone (split traces; 0 otherwise): with the profiler's per-kernel counters,
                                       instructions per step of EACH of the two launches */
    int64_t rk45_evaluated_strict_side; /* RK45: trial steps the strict side launch evaluated in full (its attempts minus replayed / extrapolated steps) */
} kr_stats;

/* PointSource<T> ctor arguments (pointsource.h:24, pointsource.cpp:11-64) */
typedef struct kr_pointsource {
    double pos[4];
    double V, spin, tol;
    double dcosalpha, dbeta;
    double cosalpha0, cosalphamax, beta0, betamax;
    double E;
} kr_pointsource;

/* ImagePlane<T> ctor arguments (imageplane.h:26, imageplane.cpp:11-121); `spin` is the PHYSICAL spin,
 * the ctor's negation is applied inside */
typedef struct kr_imageplane {
    double dist, inc_deg;
    double x0, xmax, dx;
    double y0, ymax, dy;
    double spin, phi0, precision;
} kr_imageplane;

/* radial histogram of src/emissivity/emissivity.cpp:96-126.  Per ray record:
 *   filter   steps > 0, z = r cos(theta) < 1e-2, g > 0 with g = rays[].redshift, r >= r_isco.  A ray that passes counts in disc_count, binned or not.
 *   index    q = log(r / r_min) / log(dr) (logbin) or (r - r_min) / dr, truncated toward zero like the reference's `(int) q` (emissivity.cpp:105):
 *            the ray is binned iff -1 < q < nr, at bin (int) q -- so the band -1 < q <= 0 below the first edge belongs to bin 0, as in the reference.
 *            The test is made on q itself: a NaN or out-of-range index (r_min <= 0 with logbin, dr == 0, an infinite quotient, one beyond the int
 *            range) is not binned; on-disc still counts. */
typedef struct kr_emis_bins {
    double r_min;            /* first bin edge */
    double dr;               /* logbin: ratio between edges; linear: width */
    double r_isco;           /* rays with r < r_isco are dropped */
    double gamma;            /* emis += redshift^-gamma */
    double spin;             /* unused by the filter (z = r cos(theta) only) but kept for symmetry with cartesian() */
    double num_primary_rays; /* flux += 1/(num_primary_rays * redshift) */
    int32_t nr;
    int32_t logbin;
} kr_emis_bins;

/* image accumulation of src/imageplane/imageplane_disc_image.cpp:122-161.  Per ray record:
 *   filter   steps > 0, z = r cos(theta) < 1e-2, r_isco <= r < r_disc, g > 0 with g = rays[].redshift
 *   pixel    qx = (alpha - x0) / img_dx, qy = (beta - y0) / img_dy with alpha, beta = rays[].alpha, rays[].beta, each truncated toward zero like the
 *            reference's `(int) q` (:134-135): the ray is counted iff -1 < qx < img_nx and -1 < qy < img_ny -- the band -1 < q <= 0 below the first
 *            edge belongs to column / row 0, as in the reference -- in pixel [ix img_ny + iy], ix = (int) qx, iy = (int) qy, or with flip_image
 *            iy = img_ny - 1 - (int) qy.  The test is made on qx, qy themselves: a NaN or out-of-range index (NaN or infinite alpha / beta, one
 *            beyond the int range) is not binned, and such a ray does not count in disc_count, which counts the rays that reached a pixel. */
typedef struct kr_image_bins {
    double x0, y0, img_dx, img_dy;
    double r_isco, r_disc;
    double q1, rb1, q2, rb2, q3;   /* powerlaw3, imageplane_disc_image.cpp:20-28 */
    int32_t img_nx, img_ny;
    int32_t flip_image;
    int32_t pad;
} kr_image_bins;

/* disc -> disc returning-radiation classification, src/return_radiation/disc_source_photonfrac_r.cpp:97-126
 * (that app is stale in the reference -- it calls accessors that no longer exist -- so this follows its loop body
 * against the live Ray<T> fields: cos(alpha) is rays[].alpha, beta is rays[].beta) */
typedef struct kr_return_bins {
    double r_isco, r_disc, r_esc;
    double source_r, source_phi;
    int32_t plane_iso;       /* weight = |sin(alpha) sin(beta)| instead of 1 */
    int32_t limb;            /* weight *= 1 + 2.06 |sin(alpha) sin(beta)| */
    int32_t weight_norm;     /* ray_count accumulates the weight instead of 1 */
    int32_t pad;
} kr_return_bins;

/* Landing map of the returning radiation: for one source radius, WHERE on the disc the rays of the ring come back, with which energy shift and after
 * how long -- a weighted radial histogram of the `return` class of kr_return_bins, made in the pass that classifies the rays.  Per ray record with
 * steps > 0:
 *   g, w     g = rays[].redshift, the value after redshift(-1) (disc_source_photonfrac_r.cpp:94: emitted over received energy for a Keplerian receiver
 *            at the landing point); w the weight of kr_return_bins (plane_iso, limb; rays[].alpha holds cos(alpha)).  ray_count, return, escape and
 *            lost are accumulated exactly as kr_reduce_return_f64 accumulates them.
 *   return   theta >= pi/2, r_isco <= r < r_disc, and |r - source_r| > 0.1 source_r or |phi - source_phi| > 0.1: on_disc += 1.  Such a ray is binned
 *            iff g > 0 (a NaN fails) and -1 < q < nr with q = log(r / r_min) / log(dr) (logbin) or (r - r_min) / dr -- the quotient and index rule of
 *            kr_emis_bins, the test made on q itself, so r_min <= 0, dr == 0 and the like are not errors: a NaN quotient is not binned.
 *   binned   at ir = (int) q:  count[ir] += 1, weight[ir] += w, flux[ir] += w / g, emis[ir] += w / g^gamma, time[ir] += w t;  binned += 1.
 * Rays in the self-zone of the source are in none of the sums and not in the map, as in the reference; escaped and lost rays are not in the map.
 * Output per source: double[5 nr + 6] = [count | weight | flux | emis | time | ray_count, return, escape, lost, on_disc, binned]; counts are doubles.
 * The fractions follow a loop whose program is stale in the reference (kr_return_bins above); the planes follow the emissivity histogram's rule. */
typedef struct kr_return_map {
    kr_return_bins cls;      /* classification and ray weight: exactly kr_reduce_return_f64's */
    double r_min, dr;        /* landing-radius bins; quotient and index rule of kr_emis_bins */
    double gamma;            /* emis += w * g^-gamma */
    int32_t nr, logbin;
} kr_return_map;
#ifdef __cplusplus
static_assert(sizeof(kr_return_map) == 88, "kr_return_map is 88 bytes (raytrace_cpu_amd/capi.py ReturnMap)");
#endif

/* HealpixPointSource<T> ctor arguments (healpix_pointsource.cpp:112-172): the sky of a point source sampled by the pixels of a HEALPix sphere of
 * 12 * 4^order pixels, RING ordering, and the source either orbiting (motion 0, as PointSource) or moving radially (motion 1: V is dr/dt, the
 * emitter of JetPointSource, which the reference folds into calc_consts_from_vector(..., motion = 1)).
 *   geometry   (healpix.h: ring2xyf, xyf2loc, get_pixel_vectors, quirks kept)  pixel -> (ix, iy, face) in 32-bit integers with
 *              isqrt(x) = (int) sqrt(x + 0.5) in double;  xc = (ix + 0.5) / nside, yc = (iy + 0.5) / nside, dc = 0.5 / nside;  the four corners in the
 *              order (xc + dc, yc + dc), (xc - dc, yc + dc), (xc - dc, yc - dc), (xc + dc, yc - dc), each through
 *                jr = jrll[face] - x - y;  jr < 1: nr = jr, z = 1 - nr nr / 3;  jr > 3: nr = 4 - jr, z = nr nr / 3 - 1;  else nr = 1, z = (2 - jr) 2 / 3;
 *                tmp = jpll[face] nr + x - y, brought into [0, 8) by one +8 / one -8;  phi = (nr < 1e-15) ? 0 : (0.25 pi tmp) / nr;
 *                sinTheta = sqrt((1 - z)(1 + z));  vec = (sinTheta cos(phi + 0.05), sinTheta sin(phi + 0.05), z)   -- the fixed rotation 0.05 is the reference's;
 *              the centre is 0.25 * (((c0 + c1) + c2) + c3) per component and NOT normalised (|centre| is 0.726-0.777 at order 0, 0.9946-0.9960 at
 *              order 3).  unit_center = 1 (an extension) divides it by sqrt((x x + y y) + z z).  sin / cos of phi + 0.05 are the correctly rounded pair
 *              of the strict trace; every other operation is one IEEE operation (no contraction).
 *   layout     rays_per_pixel = 5 (the reference's): the ray of vector i of pixel pix is 5 pix + i, corners i = 0..3, centre i = 4;  rays_per_pixel = 1:
 *              ray pix is the centre (still the average of the four corners).  Both of the reference's programs read only the centres.
 *   record     zeroed; t, r, theta, phi = pos;  steps = 0;  alpha = vec[2], beta = atan2(vec[1], vec[0]) (correctly rounded).
 *   disc_source  = 1 is HealpixPointSource::set_disc_source() (healpix_pointsource.h:39-43), which healpix_disc_source_photonfrac.cpp:77 calls for its
 *              source on the disc: every ray with thetadot_sign > 0 -- it starts towards increasing theta, into the disc under the source -- gets
 *              steps = -1, the rest of its record as built.  The trace passes over such a slot and the fate pass gives it class 0, so the fractions of
 *              that program are over the rays that leave the disc, about half the sphere.
 *   constants  calc_consts_from_vector (healpix_pointsource.cpp:11-109), its association kept operation for operation, with the source-frame momentum
 *              p' = {1, v0, v1, v2} -- UNIT energy, which is what the reference's class passes -- and sin / cos / tan of pos[2] from the host's C library:
 *                motion 0, basis 0   calculate_constants' tetrad (et0, et3, e10, e13, e22 = -1 / sqrt(rhosq), e31 = sqrt(delta / rhosq)):
 *                                    tdot = p'0 et0 + p'1 e10, phidot = p'0 et3 + p'1 e13, rdot = p'3 e31, thetadot = p'2 e22
 *                motion 0, basis 1   the same tdot, phidot;  rdot = p'2 (-1 sqrt(delta / rhosq)), thetadot = p'3 (-1 / sqrt(rhosq))
 *                motion 1            et0 = 1 / sqrt(g00 + g11 V V), et1 = V et0, e12 = 1 / sqrt(rhosq), e23 = sqrt(g00 / (g03 g03 - g00 g33)),
 *                                    e20 = -(g03 / g00) e23, e30 = sqrt(-g11 / g00) V / sqrt(g00 + g11 V V), e31 = sqrt(-g00 / g11) / sqrt(g00 + g11 V V):
 *                                    tdot = p'0 et0 + p'1 e20 + p'3 e30, phidot = p'1 e23, rdot = p'0 et1 + p'3 e31, thetadot = p'2 e12
 *              then k, h, Q by :99-105 and rdot_sign = rdot > 0 ? 1 : -1 (strict, unlike PointSource), thetadot_sign = thetadot > 0 ? 1 : -1.
 *   energy     CHANGED from calc_consts_from_vector's own rule, which carries E through the sums as p' = {E, E v0, E v1, E v2}: the record holds
 *              k E, h E, Q (E E) and emit E of the unit record.  That is the reference's arithmetic at E = 1, the only value its class passes, and
 *              exactly homogeneous in E otherwise; the reference's rule is not (at E = 2.5, h and Q are up to 589 and 53 ulp from 2.5 x and 6.25 x
 *              their unit values where their terms cancel).  With it goes a refusal the reference does not have: E must be positive.
 *   emit       (the _init_emit form) motion 0: redshift_start(V, reverse) of the orbiting source, as kr_redshift_start_dev_f64 computes it on the unit
 *              record (bit for bit at E = 1).  Motion 1: the same product g_ij u^i p^j with the four-velocity of the MOVING source,
 *              u = (u_t, V u_t, 0, 0), u_t = 1 / sqrt(g00 + g11 V V), and with p = (tdot, rdot, thetadot, phidot) as the tetrad launched the photon
 *              (spatial parts negated and the metric's spin negated under reverse), not as rebuilt from k, h, Q: the rebuilding takes p^r from the
 *              null condition, the un-normalised centre vector is not null (1 - |v|^2 ~ 1e-2 at order 3), and a radially moving emitter reads p^r
 *              where an orbiting one does not (rebuilt, the centre rays' emit is off by up to 4e-2).  Both depart from the reference on purpose:
 *              HealpixPointSource::redshift_start takes the orbital frame for both motions, which for a source moving at dr/dt = 0.3 spreads the
 *              "emitted" energy over 0.587 ... 1.704 E; in the source's own frame it is E to rounding.
 *   refused    (KR_EINVAL, the field named in kr_last_error, before any device call; the metric at pos from the host's C library)  order outside 0..13
 *              (at 13, 2 pix still fits the reference's int);  motion / basis not 0 or 1;  rays_per_pixel not 1 or 5;  basis = 1 with motion = 1;
 *              E not positive (or NaN);
 *              a four-velocity that is not timelike: motion 0 with 1 - (V - omega)^2 e2psi / e2nu <= 0 or NaN, motion 1 with g00 + g11 V V <= 0 or NaN.
 *              V = -1 ("Keplerian") is refused this way: a program resolves it (kr_disc_velocity) before it fills the spec.
 * Shards: `first` and `stride` count PIXELS -- slot s of a shard holds vector s % rays_per_pixel of pixel first + (s / rays_per_pixel) stride. */
typedef struct kr_healpix_source {
    double pos[4];
    double V, spin, E;
    int32_t order;
    int32_t motion;          /* 0 orbital, 1 radial: V is dr/dt */
    int32_t basis;           /* 0, 1; motion 0 only */
    int32_t rays_per_pixel;  /* 5: the reference's layout, or 1: centres only */
    int32_t unit_center;     /* 1: normalise the centre (extension) */
    int32_t disc_source;     /* 1: set_disc_source() -- rays that start towards the disc below the source are unused slots */
} kr_healpix_source;
#ifdef __cplusplus
static_assert(sizeof(kr_healpix_source) == 80, "kr_healpix_source is 80 bytes (raytrace_cpu_amd/capi.py HealpixSource)");
#endif

/* The fate of every direction of a HEALPix source's sky (healpix_to_disc.cpp:60-84, healpix_disc_source_photonfrac.cpp:84-108), one pass over the
 * CENTRE rays of a shard after the trace: slot k of a 1-ray layout, or slot 5 k + 4 of a 5-ray layout, belongs to pixel first + k stride.
 * Per centre record, with phi and g the values after range_phi and redshift (the kr_post_ form computes and stores them, the kr_reduce_ form reads
 * rays[].phi and rays[].redshift as they are):
 *   class 0  dead       steps <= 0
 *   class 4  self-zone  only if self_zone: on the disc (the rule of class 1) and |r - source_r| <= 0.1 source_r and |phi - source_phi| <= 0.1 -- the
 *                       complement of healpix_disc_source_photonfrac.cpp:95
 *   class 1  disc       theta >= pi/2 - theta_tol and r_isco <= r < r_disc
 *   class 2  escape     not on the disc and r > r_esc
 *   class 3  lost       everything else that is live.  The tests are made on the values themselves, so a NaN falls through to lost.
 * theta_tol = 0 is the photon-fraction program's rule (:94); 1e-2 is healpix_to_disc's (:65) up to its `r > r_isco` against `r >= r_isco` here.
 * Output: double[7 npix + 6] = seven planes [class | r | theta | phi | g | t | emis](npix each), written at the pixel for EVERY pixel of the shard
 * with the record's values (emis = powerlaw3(r) / g^3 for class 1, else 0), then six tallies {live, disc, escape, lost, self, 0}, counts as doubles,
 * ADDED: zero the buffer once; shards and several launches write disjoint pixels and sum the tallies. */
typedef struct kr_healpix_map {
    double r_isco, r_disc, r_esc, theta_tol, source_r, source_phi;
    double q1, rb1, q2, rb2, q3;            /* powerlaw3, imageplane_disc_image.cpp:20-28 */
    int64_t npix;
    int32_t rays_per_pixel, self_zone;
} kr_healpix_map;
#ifdef __cplusplus
static_assert(sizeof(kr_healpix_map) == 104, "kr_healpix_map is 104 bytes (raytrace_cpu_amd/capi.py HealpixMap)");
#endif

/* Emission-line profile / reverberation transfer function from image-plane rays (the reference builds it outside its C++, in
 * python/line_from_image.ipynb, from the ENSHIFT and RADIUS planes of the image FITS file).  Per ray record, after redshift(-1, reverse=1):
 *   filter   steps > 0, z = r cos(theta) < 1e-2, r_isco <= r < r_disc, g > 0 with g = rays[].redshift (the disc-image filter of
 *            imageplane_disc_image.cpp:127-128 without the pixel-range test).  A ray that passes counts in `on_disc`.
 *   emis     powerlaw3(r) (imageplane_disc_image.cpp:20-28) when table_emis == NULL; otherwise table_emis[ir] with the emissivity app's
 *            index ir = (int) (log(r / table_r_min) / log(table_dr)) (table_logbin) or (int) ((r - table_r_min) / table_dr), truncated
 *            (emissivity.cpp:58, :106).  A ray with ir outside [0, table_nr) or a non-finite table_emis[ir] passes the filter but is not binned.
 *   E, w, tau   E = line_energy / g;  w = emis * g^(-g_index);  tau = t + table_time[ir] - t0 (the table_time term is 0 without that table).
 *   bins     i = floor((E - e_min) / de), or floor(log(E / e_min) / log(de)) with log_e;  j = floor(tau / dt), or 0 without a time axis
 *            (nt == 1 and dt <= 0).  A NaN index or one outside [0, ne) / [0, nt) is not binned.
 * Output: double[2 nt ne + 2] = [count (nt x ne, time-major: [j ne + i]) | flux = sum of w (nt x ne) | on_disc | binned]; counts are doubles.
 * The per-pixel form (kr_line_from_image_dev_f64) reads the raw-sum planes of kr_reduce_image_dev_f64 / kr_post_image_dev_f64: for each pixel with
 * nrays > 0 (which counts in on_disc), with means e = enshift / nrays (the mean of 1/g), r = r / nrays, t = time / nrays: E = line_energy e,
 * w = emis(r) e^g_index, tau = t (+ table_time[ir]) - t0; same bin rules.  The call copies the table to the device once per distinct table; the copy
 * stays there while the device's table cache has room and is freed only when no call holds it and the device has drained (or by kr_shutdown). */
typedef struct kr_line_bins {
    double line_energy;            /* rest-frame line energy (e.g. 6.4) */
    double e_min, de;              /* energy bins; log_e: de is the ratio between edges */
    double t0, dt;                 /* time bins; dt <= 0 (and nt == 1): no time axis */
    double r_isco, r_disc;         /* disc filter of imageplane_disc_image.cpp:127-128 */
    double q1, rb1, q2, rb2, q3;   /* powerlaw3 emissivity (imageplane_disc_image.cpp:20-28), used when table_emis == NULL */
    double g_index;                /* weight exponent: 3 = the notebook's enshift**3 and the FLUX plane's 1/g^3 */
    double table_r_min, table_dr;  /* optional radial table, binned like kr_emis_bins (emissivity.cpp:58, :106) */
    const double* table_emis;      /* HOST, table_nr values, or NULL */
    const double* table_time;      /* HOST, table_nr values (source->disc delay), or NULL */
    int32_t ne, nt, log_e, table_nr, table_logbin, pad;
} kr_line_bins;
#ifdef __cplusplus
static_assert(sizeof(kr_line_bins) == 160, "kr_line_bins is 160 bytes (raytrace_cpu_amd/capi.py LineBins)");
#endif

/* The angle at which a photon meets the disc, in the rest frame of the orbiting gas.  For a record with steps > 0 the observer is the one of
 * kr_redshift_dev_f64(spin, V, reverse, projradius, motion = 0), quirks included: the metric takes a = reverse ? -spin : spin, the momentum p comes
 * from the constants of motion (k, h, Q, the two signs) with `spin`, its spatial part negated with reverse, and V == -1 means Keplerian at the record's r.
 * On the reference's Tetrad (kerr.h:127-170: e_t, e1 along phi, e2 along theta, e3 along r) the frame components are
 *   E = g(p, e_t)  (the `recv` of redshift(), to the bit),   P_phi = -g(p, e1),   P_th = -g(p, e2) = rho thetadot,   P_r = -g(p, e3) = rdot rho / sqrt(delta)
 * and the two angles
 *   mu  = |P_th| / E          the cosine of the angle to the disc normal, in [0, 1]
 *   chi = atan2(P_phi, P_r)   the azimuth about the normal: 0 radially outward, +pi/2 along the orbital motion.
 * A record is BAD-ANGLE when mu is not finite, mu > 1 or E <= 0.  Such records exist in the reference's own results: a ray that the integrator has
 * stepped past a radial turning point has rdot^2 < 0 under the sqrt(|.|) of the momentum, and its state is not a null vector.
 * kr_limb_law: the weight of the emission angle in the line.  law 0: 1 (isotropic);  1: 1 + coeff mu (Laor: coeff 2.06);  2: log(1 + 1 / mu)
 * (limb brightening).  Any other law is refused. */
typedef struct kr_limb_law {
    double coeff;
    int32_t law, pad;
} kr_limb_law;
/* the mu axis of the emissivity by incidence angle: nmu >= 1 equal bins of [0, 1], im = min((int) (mu nmu), nmu - 1) */
typedef struct kr_mu_bins {
    int32_t nmu, pad;
} kr_mu_bins;
#ifdef __cplusplus
static_assert(sizeof(kr_limb_law) == 16, "kr_limb_law is 16 bytes (raytrace_cpu_amd/capi.py LimbLaw)");
static_assert(sizeof(kr_mu_bins) == 8, "kr_mu_bins is 8 bytes (raytrace_cpu_amd/capi.py MuBins)");
#endif

/* A disc with a SURFACE |z| = H(rho), H(rho) = slope rho + scale (1 - sqrt(r_in / rho)): the stop_params of KR_STOP_THICKDISC, with its validation
 * (r_in positive and finite; r_out finite, <= 0: open; slope and scale non-negative and finite).  The line, the continuum, the response and the
 * per-record angles of rays that LANDED on it (kr_*_surface_* below) follow one rule per record; tests/surface_pass_rules.py restates it in numpy.
 *   observer   the one of kr_post_image_surface_dev_f64: V = -1, projradius = 1, motion = 0 -- the Keplerian gas at the cylindrical radius -- in the
 *              metric of a = reverse ? -spin : spin.  f = the frame above for that observer (E, P_r, P_th, P_phi), g = reverse ? E / emit : emit / E:
 *              redshift()'s bits.
 *   filter     steps > 0, status & KR_STATUS_DEST, g > 0, r_isco <= rho < r_disc with rho = r sin(theta) (a NaN fails); r_isco and r_disc are the
 *              bins' or the model's.  The radius that a pass hands to its item is rho: the index into an emissivity or source -> disc time table,
 *              powerlaw3, the Novikov-Thorne and ionisation zones.  t is the record's own.
 *   angle      with sn, cs = sin, cos(theta) and delta, rhosq of the metric at a, one IEEE operation per line in this association, no contraction:
 *                z = r cs;  sg = z < 0 ? -1 : 1
 *                Hp = slope + (scale 0.5 sqrt(r_in / rho)) / rho                                  H'(rho): KR_STOP_THICKDISC's step limit has the expression
 *                f_r = sg cs - Hp sn;   f_th = -(sg (r sn)) - Hp (r cs)                           the gradient of sg z - H(rho) in r and theta
 *                n_r = sqrt(delta / rhosq) f_r;   n_th = f_th / sqrt(rhosq)                       on the frame's legs e3 and e2
 *                nn = sqrt(n_r n_r + n_th n_th)
 *                P_n = (n_r P_r + n_th P_th) / nn;          mu  = |P_n| / E                        the cosine to the surface normal
 *                P_s = sg (n_r P_th - n_th P_r) / nn;       chi = atan2(P_phi, P_s)                the azimuth about it, 0 along the surface away from the axis
 *              The gas moves in phi only and the surface depends on neither t nor phi, so n is orthogonal to the gas four-velocity and the boost leaves
 *              e2 and e3 alone: this is the proper normal in the gas frame, not a flat-space approximation.  At theta = pi / 2 with Hp = 0 it is
 *              |P_th| / E and atan2(P_phi, P_r).  A ray that entered through the vertical wall at r_in or r_out is treated with the local Hp like any other.
 *   bad-angle  mu not finite, mu > 1, E <= 0, or nn not finite or zero.  Counted, and dropped under a limb law that needs the angle, as on the flat disc.
 * Not covered: the hot spot, the Stokes passes and KR_V_PLUNGE on a surface, kr_post_emissivity_mu_dev_f64 on a surface, higher-order images, f32. */
typedef struct kr_disc_surface {
    double r_in, r_out, slope, scale;
} kr_disc_surface;
#ifdef __cplusplus
static_assert(sizeof(kr_disc_surface) == 32, "kr_disc_surface is 32 bytes (raytrace_cpu_amd/capi.py DiscSurface)");
#endif

/* The polarisation of disc emission seen on a distant image plane.  The records are an image plane's (reverse = 1), the gas is the orbiting observer
 * above (motion = 0), the observer sits at inclination i = inc_deg pi / 180; sin(i) is taken once on the host.
 *   frame      exactly the one above: a = reverse ? -spin : spin, the metric g(a) at the record's (r, theta), the Tetrad legs e_t, e1 (phi), e2 (theta),
 *              e3 (r), p from the constants of motion with `spin`, its spatial part negated; E, P_r, P_th, P_phi, mu (E and mu to the bit)
 *   emitted    the polarisation vector lies in the disc plane, perpendicular to the projection of the photon direction (Chandrasekhar's orientation; a
 *              negative degree turns it by 90 degrees):  nrm = sqrt(P_r P_r + P_phi P_phi),  f = (P_phi e3 - P_r e1) / nrm,  in coordinates
 *              f^t = -P_r e1^t / nrm,  f^r = P_phi e3^r / nrm,  f^theta = 0,  f^phi = -P_r e1^phi / nrm;  g(f, p) = 0 and g(f, f) = -1 by construction
 *   transport  the Walker-Penrose constant, conserved along the null geodesic; with s = sin(theta), c = cos(theta)
 *              A = (p^t f^r - p^r f^t) + a s^2 (p^r f^phi - p^phi f^r)
 *              B = ((r^2 + a^2) (p^phi f^theta - p^theta f^phi) - a (p^t f^theta - p^theta f^t)) s
 *              kappa1 = r A - a c B,   kappa2 = -(r B + a c A)          i.e. kappa = (A - iB)(r - i a cos theta);  kappa1^2 + kappa2^2 = Q + (L - a E)^2
 *   observer   with x = rays[].alpha, y = rays[].beta:  al = -x, be = -y (the plane gives pixel (x, y) the impact parameters (-x, -y): h = -x sin(i),
 *              thetadot_sign = sign(y)),  nu = -(al + a sin(i)),  d = nu^2 + be^2,
 *              f_al = (be kappa2 - nu kappa1) / d,   f_be = (be kappa1 + nu kappa2) / d,
 *              c2 = (f_al^2 - f_be^2) / (f_al^2 + f_be^2),   s2 = 2 f_al f_be / (f_al^2 + f_be^2)
 *              = cos(2 psi), sin(2 psi) of the polarisation angle psi, measured from the image's x axis towards its y axis (the half-turn from (al, be)
 *              to (x, y) keeps angles modulo pi).  Sign convention: far from the hole a vector along e_phi comes out as (f_al, f_be) = (1, 0), one along
 *              -e_theta as (0, 1).
 * A record is BAD-POL when it is bad-angle, nrm == 0, or any of kappa1, kappa2, c2, s2 is not finite.
 * kr_pol_law: the emitted degree delta(mu).  law 0: delta = coeff;  1: delta = coeff (1 - mu) / (1 + 3.582 mu) -- with coeff = 0.1171 the usual fit to
 * Chandrasekhar's pure-scattering atmosphere (both numbers quoted from memory of the literature, not re-derived here).  Any other law, a non-finite coeff
 * and |coeff| > 1 are refused. */
typedef struct kr_pol_law {
    double coeff;
    int32_t law, pad;
} kr_pol_law;
#ifdef __cplusplus
static_assert(sizeof(kr_pol_law) == 16, "kr_pol_law is 16 bytes (raytrace_cpu_amd/capi.py PolLaw)");
#endif

/* Continuum spectrum of the disc from image-plane rays: a multicolour blackbody (what kerrbb computes) or any tabulated rest-frame spectrum (a
 * reflection table, a cut-off power law) smeared by the rays.  Where kr_line_bins puts a ray into ONE energy bin, here every disc ray adds to EVERY
 * output energy.  Per ray record, after redshift(V, reverse, projradius, motion):
 *   filter   the one of kr_line_bins: steps > 0, r cos(theta) < 1e-2, r_isco <= r < r_disc, g > 0 with g = rays[].redshift (E_rest = g E_obs, as the
 *            line uses it).  A ray that passes counts in `on_disc`.
 *   energies ne points; E_i is the CENTRE of bin i of the grid (e_min, de, log_e) of kr_line_bins: E_i = e_min + (i + 0.5) de, or the geometric
 *            centre E_i = e_min de^(i + 0.5) with log_e.  The spectrum is SAMPLED at E_i, not integrated over the bin.
 *   sum      flux[i] += w g^-3 I_rest(g E_i)  for every i (invariance of I / E^3; g^-3 = 1 / (g g g)).  Every ray is an equal image-plane pixel: the
 *            solid-angle factor dx dy / D^2 is the caller's.
 *   limb     limb(mu) of kr_limb_law, mu from the frame evaluation that gives g.  A bad-angle ray that passed the filter counts in `bad_angle`; with
 *            law != 0 it is not used, with law 0 it is used like every other ray.  The reduce forms are isotropic (law 0, no mu, bad_angle = 0).
 *   ir       the truncated radial-table index of kr_line_bins: fi = log(r / table_r_min) / log(table_dr) (table_logbin) or (r - table_r_min) / table_dr,
 *            ir = (int) fi for fi in (-1, table_nr); outside: no ir.
 * model 0, thermal:  I_rest(E') = f_col^-4 E'^3 / expm1(E' / (f_col kT)),  kT = table_kt[ir] (the units of E),  w = limb(mu).  A ray without ir, or
 *            whose kT is not finite or not positive, passes the filter but is not used.  (The kernel multiplies E' by 1 / (f_col kT), rounded once per
 *            ray; the rays' common factor f_col^-4 multiplies w g^-3.)
 * model 1, table:    I_rest(E') = S_z(E'),  w = emis(r) limb(mu),  emis = powerlaw3(r), or table_emis[ir] when table_emis != NULL -- a ray without
 *            ir or with a non-finite table_emis[ir] is not used: exactly the line's emissivity.
 *            S is a host array [nz][s_ne] on a log-energy grid: node k at s_e_min s_de^k, s_de > 1.  Linear interpolation in log E' between neighbouring
 *            nodes; exactly 0 for E' < s_e_min or E' > s_e_last = s_e_min pow(s_de, s_ne - 1) (in double, taken once): the last node itself is inside.
 *            The node position is p = u_g + u_i with u_g = log(g) / log(s_de) per ray and u_i = (log(E_i) - log(s_e_min)) / log(s_de) per energy,
 *            each taken once; p clamped to [0, s_ne - 1], k = min((int) p, s_ne - 2), S_z(E') = S[z][k] + (p - k) (S[z][k + 1] - S[z][k]).
 *            z is the radial zone (ionisation gradients): nz >= 1 zones, log-spaced over [r_isco, r_disc):
 *            z = (int) (nz log(r / r_isco) / log(r_disc / r_isco)), clamped to [0, nz - 1].
 * A ray that adds to the sums counts in `used`.
 * Output: double[ne + 4] = [flux (ne) | on_disc | used | bad_angle | 0], ADDED into: shards, several planes and several calls sum.
 * Refused (KR_EINVAL): a null model, ne < 1 or ne > 4096, de <= 0, log_e with de <= 1 or e_min <= 0, an unknown model, a non-finite parameter;
 * model 0 without table_kt, with table_nr < 1 or f_col <= 0; model 1 with s == NULL, s_ne < 2, s_de <= 1, s_e_min <= 0, nz < 1, nz s_ne > 2^20, or
 * table_emis with table_nr < 1.  The tables are copied to the device once per distinct contents (the table cache of kr_line_bins).
 *
 * STOKES SPECTRA of the continuum (kr_post_spectrum_stokes_dev_f64, kr_reduce_spectrum_stokes_*): the energy-resolved linear polarisation, Q(E) and
 * U(E) beside I(E) -- what an X-ray polarimeter measures of a thermal disc or a reflection table.  Everything of the rule above stands: filter, energies,
 * ir, zones, both models, the table interpolation, what makes a ray usable.  Everything of the kr_pol_law rule stands too: frame, emitted vector,
 * Walker-Penrose constant, observer inversion with inc_deg, c2, s2, bad-pol, the degree law delta(mu); reverse = 1 and motion = 0, as there.  What joins
 * them, per record after redshift and range_phi:
 *   on_disc  a record that passes the filter counts in `on_disc`.
 *   bad_pol  an on-disc record that is bad-pol counts in `bad_pol` and adds to nothing, WHATEVER THE LIMB LAW (as in the Stokes image, line and hot-spot
 *            passes).  Bad-angle is a subset of bad-pol: there is no separate bad_angle tally.
 *   used     otherwise limb = limb(mu) with the polarisation frame's mu (frame_value's to the bit), and the model's own rule decides: no ir, a kT that
 *            is not finite or not positive, a non-finite table_emis[ir] -> not used.  A record that adds to the sums counts in `used`.
 *   weights  c is the item word w g^-3 as the spectrum pass forms it: with g3 = 1 / ((g g) g), thermal c = (limb g3) f_col^-4 (f_col^-4 =
 *            1 / (((f f) f) f), once on the host), table c = (emis limb) g3.  Then cd = c delta(mu), cq = cd c2, cu = cd s2.
 *   sums     for every energy i, E' = g E_i and ONE X = I_rest without its common factor:
 *              thermal  X = ((E' E') E') / expm1(E' q),  q = 1 / (f_col kT) rounded once per ray
 *              table    X = S[z][k] + (p - k) (S[z][k + 1] - S[z][k]), exactly 0 (nothing added) outside [s_e_min, s_e_last]
 *            then  I[i] += c X,  Q[i] += cq X,  U[i] += cu X, each product and each sum rounded separately.  (The thermal I differs from the spectrum
 *            pass's flux in the last bit: that pass divides (c E'^3) by the expm1, this one multiplies c by the quotient.)
 *   axes     Q and U refer to the plane's own x and y axes, as in kr_post_image_stokes_dev_f64.
 * Output: double[3 ne + 4] = [I (ne) | Q (ne) | U (ne) | on_disc | used | bad_pol | 0], ADDED into: shards, several planes and several calls sum.  The
 * polarisation degree sqrt(Q^2 + U^2) / I and the angle atan2(U, Q) / 2 are the caller's to take.  ne in 1 ... 4096, as above.
 * The reduce forms take records that carry their redshift (g is READ from the record) and recompute the frame of the on-disc records for mu, c2, s2
 * and bad-pol: unlike kr_reduce_spectrum_* they take a limb law.
 * Not covered: the plunging flow (KR_V_PLUNGE is refused: polar_value has no Gram-Schmidt form), Q and U of the reverberation response, Q and U on the
 * thick-disc surface (I(E) has it: kr_post_spectrum_surface_dev_f64, kr_disc_surface above), higher-order images, f32 records, a second pass for returning radiation. */
typedef struct kr_spectrum_model {
    double e_min, de;              /* output energies: the centres of these bins; log_e: de is the ratio between edges */
    double r_isco, r_disc;         /* disc filter; the span of the zones */
    double q1, rb1, q2, rb2, q3;   /* powerlaw3 emissivity (model 1 without table_emis) */
    double f_col;                  /* colour-correction factor (model 0) */
    double table_r_min, table_dr;  /* the radial table of table_kt / table_emis, binned like kr_emis_bins */
    double s_e_min, s_de;          /* model 1: first node and node ratio of the rest-frame grid */
    const double* table_kt;        /* HOST, table_nr values of kT (model 0) */
    const double* table_emis;      /* HOST, table_nr values, or NULL: powerlaw3 (model 1) */
    const double* s;               /* HOST, nz x s_ne values (model 1) */
    int32_t model, ne, log_e, table_nr, table_logbin, s_ne, nz, pad;
} kr_spectrum_model;
#ifdef __cplusplus
static_assert(sizeof(kr_spectrum_model) == 168, "kr_spectrum_model is 168 bytes (raytrace_cpu_amd/capi.py SpectrumModel)");
#endif

/* An orbiting hot spot on the disc, seen on an image plane: the light curve, the flux-weighted image position and the energy-time spectrogram of a line
 * emitted by the spot.  The spot is a PATTERN of enhanced emission on the disc surface, centred at radius r_spot, at azimuth phi0 at coordinate time 0,
 * moving at the pattern speed Om.  The gas under it stays on its Keplerian orbits: g, mu and bad-angle are exactly what the redshift / limb passes give
 * today.  It is not a rigid body with a four-velocity of its own, and the rule is good for sigma << r_spot only.
 * Time and sense of rotation: an image plane is traced backwards by negating the spin, so a record's t grows into the past and its phi is the true
 * azimuth.  A photon that reaches the observer at time T left the disc at T - rays[].t, when the spot stood at phi0 + Om (T - rays[].t).  With
 * a' = reverse ? -spin : spin (the a' of the redshift pass, i.e. the true spin), Om > 0 is prograde for a' > 0.
 * Per ray record, after redshift(V, reverse, projradius, motion) and range_phi(lo, hi):
 *   filter   the one of kr_line_bins: steps > 0, r cos(theta) < 1e-2, r_isco <= r < r_disc, g > 0 with g = rays[].redshift (E_rest = g E_obs).  A ray that
 *            passes counts in `on_disc`.
 *   limb     limb(mu) of kr_limb_law, as in kr_spectrum_model: a bad-angle ray that passed the filter counts in `bad_angle`; with law != 0 it is dropped,
 *            with law 0 it is used like every other ray.  The reduce forms are isotropic (law 0, no mu, bad_angle = 0).
 *   ring     fabs(r - r_spot) < cut sigma, the product rounded once: a necessary condition for a non-zero contribution.  A ray that passes counts in
 *            `used`.
 *   Om       omega when shear == 0.  With shear == 1, Om = 1 / (a_orbit + r sqrt(r)): each radius moves at its own Keplerian rate and the spot winds
 *            into an arc.  omega == 0 is a static pattern.
 *   weight   c = limb pow(g, -g_index): g_index 4 gives the bolometric intensity, 3 the specific intensity of a line, as the line pass uses it.
 *   energy   only with ne > 0: E = line_energy / g on the grid (e_min, de, log_e) with the index rule of kr_line_bins, ie = floor((E - e_min) / de) or
 *            floor(log(E / e_min) / log(de)).  A NaN index or one outside [0, ne): the ray adds to no spectrogram cell, but still to the light curve.
 *   samples  for every T_k = t0 + k dt, k = 0 .. nt - 1 (SAMPLED, not integrated over the step):
 *              d2 = r r + r_spot r_spot - 2 r r_spot cos(phi - (phi0 + Om (T_k - t)))
 *              s  = exp(-d2 / (2 sigma sigma)) - exp(-cut cut / 2)
 *              if s > 0:  flux[k] += c s,  sx[k] += c s x,  sy[k] += c s y  (x = rays[].alpha, y = rays[].beta),  spec[k][ie] += c s
 *            The Gaussian is SHIFTED: s is continuous and reaches 0 at d = cut sigma, so a last-bit difference in d2 moves a sum by a last-bit amount and
 *            never adds or removes a whole term.  (The kernel multiplies d2 by -1 / (2 sigma sigma), rounded once.)
 * Output: double[nt (3 + ne) + 4] = [flux (nt) | sx (nt) | sy (nt) | spec (nt x ne, time-major: [k ne + ie]) | on_disc | used | bad_angle | 0], ADDED
 * into: shards, several planes, several spots and several calls sum.  The centroid sx / flux, sy / flux is the caller's to take.
 * Refused (KR_EINVAL): a null spot; a non-finite parameter; nt < 1 or nt > 4096; ne < 0 or ne > 4096; nt ne > 2^20; sigma <= 0; cut <= 0; r_spot <= 0;
 * with ne > 0: de <= 0, log_e with de <= 1 or e_min <= 0, line_energy <= 0; shear other than 0 or 1; with shear == 1, a_orbit + r_isco sqrt(r_isco) <= 0.
 * The struct holds no host pointer: nothing goes through the table cache.  The pad words are reserved and not judged.
 *
 * STOKES LIGHT CURVES of the spot (kr_post_hotspot_stokes_dev_f64, kr_reduce_hotspot_stokes_*): the time-resolved linear polarisation, Q[k] and U[k]
 * beside flux, sx, sy.  Everything of the rule above stands: filter, ring, Om, the weight c = limb g^-g_index, the energy bin, the samples T_k, the shifted
 * Gaussian s.  Everything of the kr_pol_law rule stands too: frame, emitted vector, Walker-Penrose constant, observer inversion with inc_deg, c2, s2,
 * bad-pol, the degree law delta(mu); reverse = 1 and motion = 0, as there.  mu of the limb law and of delta is that frame's.  What joins them:
 *   bad-pol  a record that passes the filter and the ring and is NOT bad-pol counts in `used`.  One that passes both and IS bad-pol counts in `bad_pol`
 *            and adds to nothing, whatever the limb law (as in the Stokes image and line passes, where bad-pol rays are never binned).  Bad-angle is a
 *            subset of bad-pol: there is no separate bad_angle tally.  A bad-pol record outside the ring is not counted.
 *   sums     for every sample with s > 0:  flux[k] += c s,  sx[k] += c s x,  sy[k] += c s y,  Q[k] += ((c delta) c2) s,  U[k] += ((c delta) s2) s,  and with
 *            ne > 0  spec[k][ie] += c s  (intensity only: there is no Q, U spectrogram)
 *   axes     Q and U refer to the plane's own x and y axes, as in kr_post_image_stokes_dev_f64
 * Output: double[nt (5 + ne) + 4] = [flux | sx | sy | Q | U (nt each) | spec (nt x ne, time-major) | on_disc | used | bad_pol | 0], ADDED into.  The
 * polarisation degree sqrt(Q^2 + U^2) / flux and the angle atan2(U, Q) / 2 are the caller's to take.
 * The reduce forms take records that carry their redshift and wrapped phi (g and phi are READ from the record) and recompute the frame of the ring
 * records for mu, c2, s2 and bad-pol: unlike kr_reduce_hotspot_* they take a limb law.
 * Not covered: Q, U spectrograms, the plunging flow (KR_V_PLUNGE is refused), the thick-disc surface, higher-order images, f32 records. */
typedef struct kr_hotspot {
    double r_spot, sigma, cut;     /* centre radius, Gaussian width and the cut-off in units of sigma */
    double phi0, omega;            /* azimuth at coordinate time 0; pattern speed (shear == 0) */
    double a_orbit;                /* the spin of the Keplerian rate under shear == 1 */
    double t0, dt;                 /* observer times T_k = t0 + k dt */
    double g_index;                /* weight exponent: c = limb g^-g_index */
    double line_energy;            /* rest-frame line energy of the spectrogram (ne > 0) */
    double e_min, de;              /* energy bins of the spectrogram; log_e: de is the ratio between edges */
    double r_isco, r_disc;         /* disc filter */
    int32_t nt, ne, log_e, shear, pad[2];
} kr_hotspot;
#ifdef __cplusplus
static_assert(sizeof(kr_hotspot) == 136, "kr_hotspot is 136 bytes (raytrace_cpu_amd/capi.py HotSpot)");
#endif

/* Reverberation response of the disc from image-plane rays: the energy-time impulse response of a whole tabulated rest-frame reflection spectrum (iron
 * line, soft excess and Compton hump together, ionisation zones included).  Where kr_line_bins bins ONE line into (time, energy) and kr_spectrum_model
 * smears a spectrum into every output energy with no time axis, here every disc ray adds to EVERY energy of ONE time row.  `spec` must be the table
 * model (spec.model == 1); the thermal model is refused.  Per ray record, after redshift(V, reverse, projradius, motion):
 *   filter, limb, ir, zone, emis, w, S_z(g E_i)
 *            exactly as kr_spectrum_model states them for model 1, quoted:
 *              "filter   the one of kr_line_bins: steps > 0, r cos(theta) < 1e-2, r_isco <= r < r_disc, g > 0 with g = rays[].redshift (E_rest = g E_obs, as
 *                        the line uses it).  A ray that passes counts in `on_disc`."
 *              "limb     limb(mu) of kr_limb_law, mu from the frame evaluation that gives g.  A bad-angle ray that passed the filter counts in `bad_angle`;
 *                        with law != 0 it is not used, with law 0 it is used like every other ray.  The reduce forms are isotropic (law 0, no mu,
 *                        bad_angle = 0)."
 *              "ir       the truncated radial-table index of kr_line_bins: fi = log(r / table_r_min) / log(table_dr) (table_logbin) or
 *                        (r - table_r_min) / table_dr, ir = (int) fi for fi in (-1, table_nr); outside: no ir."
 *              "model 1, table:    I_rest(E') = S_z(E'),  w = emis(r) limb(mu),  emis = powerlaw3(r), or table_emis[ir] when table_emis != NULL -- a ray
 *                        without ir or with a non-finite table_emis[ir] is not used: exactly the line's emissivity."  S, its nodes, the interpolation, the
 *                        zeros outside [s_e_min, s_e_last] and the zone z: as that comment goes on to state them.
 *            ir is needed when table_emis OR table_time is present.  A record without ir, or with a non-finite table_time[ir], passes the filter but
 *            is not used.
 *   time     ft = (t + tt - t0) / dt with t = rays[].t (disc -> observer) and tt = table_time ? table_time[ir] : 0 (source -> disc): the same
 *            expression, in the same order, as the line pass.  j = (int) floor(ft).  A used record whose ft is NaN or outside [0, nt) counts in `outside`
 *            and adds nothing.
 *   sum      resp[j ne + i] += w g^-3 S_z(g E_i)  for every i (E_i: the bin centres of spec's grid, as kr_spectrum_model samples them).
 * Output: double[nt ne + 4] = [resp (nt x ne, time-major: [j ne + i]) | on_disc | used | bad_angle | outside], ADDED into: shards, several planes and
 * several calls sum.  `used` counts the records that pass every test except the time window; `outside` is a subset of `used`.
 * Refused (KR_EINVAL): everything kr_spectrum_model refuses of spec; spec.model != 1; nt < 1; dt not positive or not finite; a non-finite t0;
 * nt ne > 2^24; table_time with table_nr < 1 (or a non-finite table_r_min / table_dr).  table_time needs no table_emis (powerlaw3 then gives emis).
 * The tables are copied to the device once per distinct contents (the table cache of kr_line_bins). */
typedef struct kr_response_model {
    kr_spectrum_model spec;        /* model 1: the rest-frame spectrum, its zones, the emissivity, the output energies, the disc filter */
    double t0, dt;                 /* time rows: row j holds t0 + j dt <= t + tt < t0 + (j + 1) dt */
    const double* table_time;      /* HOST, spec.table_nr values of the source -> disc time by radius (spec's radial table), or NULL: no source delay */
    int32_t nt, pad;
} kr_response_model;
#ifdef __cplusplus
static_assert(sizeof(kr_response_model) == 200, "kr_response_model is 200 bytes (raytrace_cpu_amd/capi.py ResponseModel)");
#endif

/* Critical-curve (caustic) maps of the disc on an image plane: src/caustic/caustic_discplane.cpp.  Per image-plane pixel (ix, iy), from the ray through
 * the pixel (bundle mode: member 0 of its 5-ray bundle, imageplane_bundles.h) after redshift(dest, reverse) (caustic_discplane.cpp:219-251):
 *   valid_hit   steps > 0, r_isco <= r < r_disc, redshift > 0 (:177-182)
 *   on a hit    HIT = 1, RADIUS = r, PHI = phi_s = atan2(sin phi, cos phi) of the accumulated phi, X_DISC = r cos phi_s, Y_DISC = r sin phi_s,
 *               ORDER = max((int) (|phi| / 2 pi), rdot_flips / 2), REDSHIFT = redshift; otherwise zeros and ORDER = -1
 *   DET_J, SIGN_J   bundles = 1 (:279-334): NaN, 0 unless the centre and its four satellites (east, west, north, south at +- eps_x, +- eps_y) are
 *               valid hits; 1e30, 0 unless all four have the centre's rdot_flips and an accumulated phi within pi / 2 of its; otherwise the
 *               determinant of the central differences of (X_DISC, Y_DISC) over 2 eps_x, 2 eps_y and its sign (+1 / -1 / 0).
 *               bundles = 0 (:403-439): the same from the X_DISC / Y_DISC planes of the four neighbouring pixels over 2 eps_x, 2 eps_y (here the
 *               spacing of the ray grid), with HIT / ORDER of the neighbours in place of the satellite tests; border pixels stay NaN, 0.
 * d_maps: 9 nx ny + 7 doubles on the device, [DET_J | SIGN_J | ORDER | HIT | RADIUS | PHI | X_DISC | Y_DISC | REDSHIFT], each [ix ny + iy] like
 * Array2D, then disc_count, horizon, rlim, steplim, out_of_range, other (the diagnostic counts of :255-276 over the centre rays), suppressed. */
typedef struct kr_caustic_map {
    double r_isco, r_disc;         /* valid_hit */
    double eps_x, eps_y;           /* bundles = 1: satellite offsets;  bundles = 0: dx, dy of the ray grid */
    int32_t nx, ny;                /* pixels = bundle centres (fencepost counts) */
    int32_t bundles;               /* 1: 5 records per pixel;  0: one record per pixel + neighbour differences */
    int32_t pad;
} kr_caustic_map;
#ifdef __cplusplus
static_assert(sizeof(kr_caustic_map) == 48, "kr_caustic_map is 48 bytes (raytrace_cpu_amd/capi.py CausticMap)");
#endif

/* Caustic maps of the source sphere (src/caustic/caustic_sourceplane.cpp: rays run free, theta_max = 0, to the sphere r = r_lim; det J of
 * d(theta_s, phi_s) / d(x_img, y_img)) and of a flat source plane behind the hole (src/caustic/caustic_plane.cpp: rays stop on a
 * FlatPlaneDestination; det J of d(x_s, y_s) / d(x_img, y_img)).  Per image-plane pixel (ix, iy), from the ray through the pixel (bundle mode:
 * member 0 of its 5-ray bundle), as it comes out of the trace -- no redshift, no range_phi:
 *   kind = 0    ESCAPED = steps > 0 && (status & KR_STATUS_RLIM) (caustic_sourceplane.cpp:191); then THETA_S = theta, PHI_S = atan2(sin phi, cos phi)
 *               of the accumulated phi, ORDER = max(floor(|phi| / pi) - 1, 0) (:202-219); otherwise NaN, NaN, -1 (:225-228)
 *   kind = 1    HIT_PLANE = steps > 0 && (status & KR_STATUS_DEST) (caustic_plane.cpp:187-189); then (X_S, Y_S) = source_coords(r, theta, phi)
 *               (ray_destination.h:195-203: X = r sin theta cos phi, Y = r sin theta sin phi, Z = r cos theta, X_S = -X sin phi0 + Y cos phi0,
 *               Y_S = -X cos incl cos phi0 - Y cos incl sin phi0 + Z sin incl), ORDER = max((int) (|phi| / 2 pi), rdot_flips / 2) (:180-184);
 *               otherwise NaN, NaN, -1 (:232-238).  The caller evaluates the four sines and cosines with the C library, as the reference does.
 *   RDOT_FLIPS, EQUAT_CROSS   rdot_flips, equatorial_crossings of that ray, whatever became of it
 *   DET_J, SIGN_J   bundles = 1 (kind = 1 only; caustic_plane.cpp:249-299): NaN, 0 unless the centre and its four satellites (east, west, north, south at
 *               +- eps_x, +- eps_y) are hits; 1e30, 0 unless all four have the centre's rdot_flips and an accumulated phi within pi / 2 of its;
 *               otherwise the determinant of the central differences of (X_S, Y_S) over 2 eps_x, 2 eps_y and its sign (+1 / -1 / 0).
 *               bundles = 0 (caustic_sourceplane.cpp:264-305, caustic_plane.cpp:357-392): the same from the two coordinate planes of the four
 *               neighbouring pixels over 2 eps_x, 2 eps_y (here the spacing of the ray grid), with their ESCAPED / HIT_PLANE and ORDER in place of
 *               the satellite tests; border pixels stay NaN, 0.  kind = 0 wraps the two PHI_S differences into [-pi, pi] (wrap_dphi, :68-73).
 * d_maps: 8 nx ny + 3 doubles on the device, [DET_J | SIGN_J | ORDER | ESCAPED or HIT_PLANE | THETA_S or X_S | PHI_S or Y_S | RDOT_FLIPS |
 * EQUAT_CROSS], each [ix ny + iy] like Array2D, then the three counts over the rays through the pixels: escaped or hit, captured (KR_STATUS_HORIZON
 * among the others), steplim (steps <= 0 or KR_STATUS_STEPLIM). */
typedef struct kr_source_map {
    int32_t kind;                  /* 0: source sphere;  1: flat source plane */
    int32_t bundles;               /* 1: 5 records per pixel (kind = 1 only);  0: one record per pixel + neighbour differences */
    int32_t nx, ny;                /* pixels = bundle centres (fencepost counts) */
    double eps_x, eps_y;           /* bundles = 1: satellite offsets;  bundles = 0: dx, dy of the ray grid */
    double sin_incl, cos_incl;     /* kind = 1: of the FlatPlaneDestination's incl (radians) ... */
    double sin_phi0, cos_phi0;     /* ... and phi0;  unused by kind = 0 */
} kr_source_map;
#ifdef __cplusplus
static_assert(sizeof(kr_source_map) == 64, "kr_source_map is 64 bytes (raytrace_cpu_amd/capi.py SourceMap)");
#endif

/* What run_raytrace's trajectory dump takes besides the trace parameters (raytracer.h:112-122: write_step, write_rmax, write_rmin).  A struct of
 * its own: kr_params and kr_stats keep their sizes.  write_rmin / write_rmax < 0: that side of the radial window is open. */
typedef struct kr_path_spec {
    double write_rmin, write_rmax;
    int32_t write_step, pad;
} kr_path_spec;
#ifdef __cplusplus
static_assert(sizeof(kr_path_spec) == 24, "kr_path_spec is 24 bytes (raytrace_cpu_amd/capi.py PathSpec)");
#endif

/* The (r, theta, phi) grid of a volume illumination map and the observers that measure a ray's energy shift in it (kr_trace_volume_* below has the
 * rule).  Radial edges r_min dr^i (logbin) or r_min + i dr; polar cells of dtheta from theta = 0; azimuthal cells of dphi from phi = -pi.
 * mode 0: one deposit per passage of a cell; 1: one per row (Mapper::map_ray's literal behaviour).  V, reverse, projradius, motion: as kr_redshift_dev_f64
 * takes them (V = -1, projradius = 1: the mapper's own 1 / (a + r sin(theta) sqrt(r sin(theta)))). */
typedef struct kr_volume_map {
    double r_min, dr, dtheta, dphi;
    double V;
    int32_t nr, ntheta, nphi, logbin, mode, reverse, projradius, motion;
} kr_volume_map;
#ifdef __cplusplus
static_assert(sizeof(kr_volume_map) == 72, "kr_volume_map is 72 bytes (raytrace_cpu_amd/capi.py VolumeMap)");
#endif

/* The energy and time bins of an observed volume map (kr_trace_observe_* below has the rule).  Energy edges en0 + i den, or en0 den^i with logbin_en;
 * time edges t0 + i dt; nt = 0: no response. */
typedef struct kr_observe_bins {
    double en0, den, t0, dt;
    int32_t nen, nt, logbin_en, pad;
} kr_observe_bins;
#ifdef __cplusplus
static_assert(sizeof(kr_observe_bins) == 48, "kr_observe_bins is 48 bytes (raytrace_cpu_amd/capi.py ObserveBins)");
#endif

/* What a crossing-recording trace takes besides the trace parameters (kr_trace_crossings_* below has the rule).  V, reverse, projradius, motion: the
 * emitter on the equatorial plane, as kr_redshift_dev_f64 takes them. */
typedef struct kr_crossing_spec {
    double  V;                 /* observer on the plane, as kr_redshift_dev_f64 takes it; -1: Keplerian at r_c */
    int32_t max_crossings;     /* M, 1..16: crossings stored per ray */
    int32_t stop_when_full;    /* 1: the ray ends with the iteration that made its M-th crossing */
    int32_t reverse, projradius, motion, pad;
} kr_crossing_spec;
#ifdef __cplusplus
static_assert(sizeof(kr_crossing_spec) == 32, "kr_crossing_spec is 32 bytes (raytrace_cpu_amd/capi.py CrossingSpec)");
#endif

/* PointSourceVel<T> ctor arguments (pointsource_vel.h, pointsource_vel.cpp:11-110): a point source whose emitter has ANY timelike four-velocity -- an
 * orbiting and outflowing corona, a blob plunging inside the ISCO, a source drifting in theta -- sampled on the (cos alpha, beta) grid of kr_pointsource.
 *   count      rays = (int) ((((cosalphamax - cosalpha0) / dcosalpha) + 1) * (((betamax - beta0) / dbeta) + 1)), the int-truncated PRODUCT of doubles (:12);
 *              n_cosalpha, n_beta the truncated factors (:15-16).  Ray ix = i n_beta + j; slots from n_cosalpha n_beta on are unused (steps = -1).
 *   tetrad     SolveTetrad (:113-260), once per call ON THE HOST in plain C++ (csrc/kr_vel_tetrad.hpp), sin / cos / tan of pos[2] from the C library, every
 *              other line one IEEE operation in the reference's association:
 *                metric    rhosq = r r + (a cos)(a cos);  delta = r r - 2 r + a a;  sigmasq = (r r + a a)(r r + a a) - a a delta sin sin;
 *                          e2nu = rhosq delta / sigmasq;  e2psi = sigmasq sin sin / rhosq;  omega = 2 a r / sigmasq;
 *                          g00 = e2nu - omega omega e2psi, g03 = g30 = omega e2psi, g11 = -rhosq / delta, g22 = -rhosq, g33 = -e2psi
 *                start     v0 = u AS GIVEN (not normalised), v1 = d_r, v2 = d_theta, v3 = d_phi -- the radial one first
 *                G-S       e_i = v_i - sum_{j<i} (g(v_i, e_j) / g(e_j, e_j)) e_j, the projections of v_i (classical Gram-Schmidt) subtracted in the order
 *                          j = 0, 1, 2;  g(x, y) = the sum over all sixteen (a, b) in row-major order, zeros included, of (g_ab x^a) y^b
 *                normalise e_i /= sqrt(|g(e_i, e_i)|), component by component
 *                permute   leg 0 = e_0, leg 3 = e_1, leg 1 = e_2, leg 2 = e_3
 *                signs     leg 1 negated if its theta component < 0, leg 2 if its phi component < 0, leg 3 if its r component < 0
 *              so leg 1 has a positive theta component, leg 2 a positive phi component, leg 3 a positive r component.  kr_pointsource_vel_tetrad returns it.
 *   record     InitPointSourceVel (:34-110) against this record, each step literal.  cosalpha = cosalpha0 + i dcosalpha, beta = beta0 + j dbeta.
 *              cosalpha >= cosalphamax or beta >= betamax: the record is zeroed with steps = -1.  DIFFERS from the reference, which RETURNS from the whole
 *              constructor at the first such ray (:50) and leaves every later ray unbuilt; here only that ray is marked, the PointSource rule
 *              (pointsource.cpp:40-44).  Otherwise the record is zeroed, then t, r, theta, phi = pos; steps = 0; alpha = cosalpha (sic, as PointSource),
 *              beta = beta; rdot_flips = equatorial_crossings = status = 0, and with alpha = acos(cosalpha):
 *                p' = {E, E sin(alpha) cos(beta), E sin(alpha) sin(beta), E cos(alpha)}        (products left to right; cos(alpha) of the acos, not cosalpha)
 *                tdot = p'0 leg0[t] + p'1 leg1[t] + p'2 leg2[t] + p'3 leg3[t], summed left to right; rdot, thetadot, phidot likewise with [r], [theta], [phi]
 *                k = (1 - 2 r / rhosq) tdot + (2 a r sin sin / rhosq) phidot
 *                h = phidot ((r r + a a)(r r + a a cos cos - 2 r) sin sin + 2 a a r sin sin sin sin);  h = h - 2 a r k sin sin;  h = h / (r r + a a cos cos - 2 r)
 *                Q = rhosq rhosq thetadot thetadot - (a k cos + h / tan)(a k cos - h / tan)
 *                rdot_sign = rdot > 0 ? 1 : -1, thetadot_sign = thetadot > 0 ? 1 : -1
 *              acos is the correctly rounded routine of csrc/kr_crmath.hpp, sin / cos of alpha and beta those of csrc/kr_sincos.hpp (on the device); sin, cos,
 *              tan of pos[2] are the host C library's values; no contraction.
 *   emit       (the _init_emit form)  the photon's energy in the emitter's OWN frame, g_ab u^a p^b:  N = g(u, u) of the input u by the sum above;
 *              un[a] = u[a] / sqrt(N) (host, four divisions);  p = (tdot, rdot, thetadot, phidot) as the tetrad launched the photon;  emit = the sum over
 *              all sixteen (a, b) in row-major order, zeros included, of (g_ab un^a) p^b, starting from 0.  It is E to rounding on every ray.
 *              DIFFERS from the reference on purpose, as the HEALPix source's moving emitter does: PointSourceVel::RedshiftStart (:263-269) calls
 *              Raytracer::RedshiftStart(velocity), the frame of an ORBIT of angular velocity `velocity` whatever the emitter's motion.
 *   refused    (KR_EINVAL, message in kr_last_error, before any device work)  a null pointer, n < 0;  n that is not the spec's ray count;  a non-finite
 *              pos or u;  u that is not timelike, g(u, u) <= 0 or NaN;  u^t <= 0;  r <= horizon = 1 + sqrt((1 - a)(1 + a)) (or a NaN horizon);  a grid whose
 *              ray count is negative, NaN or beyond int. */
typedef struct kr_pointsource_vel_spec {
    double pos[4];
    double u[4];             /* contravariant (u^t, u^r, u^theta, u^phi); need not be normalised */
    double spin, tol, E;     /* tol: carried for the constructor's signature (the trace reads kr_params) */
    double dcosalpha, dbeta;
    double cosalpha0, cosalphamax, beta0, betamax;
} kr_pointsource_vel_spec;
#ifdef __cplusplus
static_assert(sizeof(kr_pointsource_vel_spec) == 136, "kr_pointsource_vel_spec is 136 bytes (raytrace_cpu_amd/capi.py PointSourceVelSpec)");
#endif

/* Where the rays of ONE source end, by emission angle: the loop of src/return_radiation/disc_source_return_angdist.cpp:132-196 (a program that is stale
 * in the reference: it calls map_results, ray_cosalpha and ray_beta, which no longer exist) against the live record fields.  Per record with steps > 0,
 * with c = rays[].alpha (which holds cos alpha) and beta = rays[].beta:
 *   bad_g      += 1 when rays[].redshift is not > 0 (the reference does not compute it, :125-128; nothing else reads it)
 *   skipped    c == 0: skipped += 1 and nothing else (:136)
 *   angles     alpha = acos(c);  s = sin(alpha) sin(beta);  norm = acos(|s|);  az = acos(-c / sqrt(1 - s s)), negated when sin(alpha) cos(beta) < 0.
 *              acos / sin / cos are the correctly rounded routines of csrc/kr_crmath.hpp / csrc/kr_sincos.hpp.
 *   labels     The rule above is the reference's, for records of kr_pointsource (labels = 0): calculate_constants puts sin(alpha) cos(beta) on its leg
 *              along +phi and sin(alpha) sin(beta) on -theta, so |s| is the cosine of the angle to the disc normal.  SolveTetrad's leg 1 is +theta and
 *              its leg 2 +phi: the ray (alpha, beta) of kr_pointsource_vel_spec is the ray (alpha, beta - pi/2) of kr_pointsource.  labels = 1 (an
 *              extension) reads such records: sin(beta) is replaced by -1 cos(beta) and cos(beta) by sin(beta) in s and in the sign test of az --
 *              both exact -- so norm and az keep their meaning; the alpha and beta histograms bin the stored values either way.
 *   bins       Nangle = (int) (2 pi / dangle);  bin(x) = (int) q with q = (x + pi) / dangle, M_PI as a double.  The test is made on q itself, the index
 *              rule of kr_emis_bins: the ray is binned iff -1 < q < Nangle for ALL FOUR angles.  Otherwise -- a NaN angle (az at |s| = 1, or where
 *              rounding takes |c / sqrt(1 - s s)| past 1), beta outside [-pi, pi) -- out_of_range += 1 and the ray is in no histogram and no sum.
 *              DIFFERS from the reference, which would index its arrays out of bounds there.
 *   weight     w = plane_iso ? |s| : 1, times 1 + 2.06 |s| with limb (cls.plane_iso, cls.limb);  ray_count += cls.weight_norm ? w : 1
 *   totals     total_norm[bin(norm)] += 1, total_az[bin(az)] += 1 (:156-157: unweighted)
 *   class      the rule of kr_return_bins, exactly as kr_reduce_return_f64 and the landing map apply it, phi as stored:
 *                return  theta >= pi/2, r_isco <= r < r_disc, and |r - source_r| > 0.1 source_r or |phi - source_phi| > 0.1
 *                escape  not on the disc and r > r_esc;   lost  not on the disc, not escaped, r < r_isco;   anything else: other += 1
 *              (the reference has the self-zone test commented out, :161; source_r = 0 switches it off here.)  A classified ray adds w to its class sum
 *              and to hist[class][alpha][bin(alpha)], [beta][bin(beta)], [norm][bin(norm)], [az][bin(az)].
 * Output: double[14 Nangle + 8], ADDED into (zero it once; beta-halves, shards and several sources sum):
 *   [escape: alpha | beta | norm | az] [return: alpha | beta | norm | az] [lost: alpha | beta | norm | az] [total_norm | total_az]   (Nangle each)
 *   {ray_count, escape, return, lost, other, skipped, out_of_range, bad_g}                                                             (counts as doubles)
 * The per-bin normalisation of the az histograms (:200-209) is left to the caller.
 * Refused (KR_EINVAL): a null pointer, n < 0, dangle that is not positive or gives Nangle < 1 or > 4096, labels not 0 or 1. */
typedef struct kr_angdist_spec {
    kr_return_bins cls;      /* classification and ray weight: kr_reduce_return_f64's (with labels = 1 the weight's |s| is the relabelled one) */
    double dangle;
    int32_t labels;          /* 0: records of kr_pointsource (the reference's rule); 1: records of kr_pointsource_vel_spec */
    int32_t pad;
} kr_angdist_spec;
#ifdef __cplusplus
static_assert(sizeof(kr_angdist_spec) == 72, "kr_angdist_spec is 72 bytes (raytrace_cpu_amd/capi.py AngdistSpec)");
#endif

/* The source-to-observer link: the DIRECT continuum of a source, by observer inclination -- where on the sky at infinity its escaping rays go, when they
 * reach a reference sphere and with what energy.  It gives the three numbers the lag layer takes from its caller (the arrival instant t0 of the direct
 * continuum, its flux, and the reflection fraction R_f = return / escape) and covers the reference's lamppost/pointsource_sky programs.  The records
 * are those of any source (kr_pointsource, kr_pointsource_vel_spec, kr_healpix_source) traced with KR_STOP_THETA to the disc plane and out to r_max.
 * Per record with steps > 0 (in the kr_post_ form after range_phi and redshift(V, reverse, projradius, motion), whose g this rule does not read):
 *   class      the rule of kr_return_bins exactly as kr_angdist_spec applies it, phi as stored:
 *                return  theta >= pi/2, r_isco <= r < r_disc, and |r - source_r| > 0.1 source_r or |phi - source_phi| > 0.1
 *                escape  not on the disc and r > r_esc;   lost  not on the disc, not escaped, r < r_isco;   anything else: other
 *              (cls.source_r = 0 switches the self-zone off; cls.plane_iso, cls.limb and cls.weight_norm are not read: the four classes are
 *              unweighted counts here.)  ray_count += 1 and the class's tally += 1.  Only class `escape` goes further.
 *   momentum   (pt, pr, ptheta, pphi) = momentum_from_consts(k, h, Q, rdot_sign, thetadot_sign, r, theta, spin) at the record's own (r, theta), the
 *              expressions redshift() evaluates, with `spin` of this struct (the trace's kr_params.spin).  pr <= 0 (a NaN too), or any of the four
 *              not finite: inbound += 1 and nothing else.
 *   direction  Far out d theta / d r and d phi / d r fall as r^-2, so the rest of the way to infinity adds r (d theta / d r):
 *                theta_obs = theta + r * ptheta / pr;   phi_obs = phi + r * pphi / pr;   mu = cos(theta_obs)     (cos: csrc/kr_sincos.hpp)
 *              The position angle alone is off by about b / r for impact parameter b, 0.01 rad at r = 1000; this takes that first-order term out.
 *              phi_obs is part of the rule (tests/observer_rules.py returns it) and is binned nowhere.
 *   energy     For the static observer at infinity, e_t = (1, 0, 0, 0), the received energy is g_ab e_t^a p^b -> g_tt p^t -> + p^t -> + k as r -> inf:
 *              kerr_metric's g_tt = e2nu - omega^2 e2psi -> +1 (signature + - - -) and g_tphi -> 0, and p^t -> k.  So E_inf = + k, the conserved
 *              rays[].k; no metric is evaluated.  shift = E_inf / emit = k / rays[].emit, the usual g = E_obs / E_emit.  shift not > 0 (a NaN too):
 *              bad_g += 1 and nothing else.
 *   time       dist > 0: t_ref = t + (dist - r) + 2 * log(dist / r), the flat and the Shapiro term of an outgoing ray from r to the sphere r = dist (every
 *              ray stops one step past r_max, each at its own r).  dist == 0: t_ref = t.  With dist the image plane's dist, t_ref and the image-plane
 *              records' t + tt share an origin; what remains is the sphere-against-plane term b^2 / (2 dist), which is NOT corrected.
 *   weight     w = shift^gamma (pow), gamma the photon index; gamma = 0: pure solid-angle counts (every ray of the source grids carries equal solid angle).
 *   bins       q = (mu - mu0) / dmu; the ray is binned iff -1 < q < nmu, in imu = (int) q -- the index rule of kr_emis_bins, decided on the quotient.
 *              Otherwise (a NaN too) outside_mu += 1 and nothing else.  A binned ray: binned += 1 and
 *                count[imu] += 1;  sum_w[imu] += w;  sum_ws[imu] += w * shift;  sum_wt[imu] += w * t_ref
 *              nt > 0: ft = (t_ref - t0) / dt; 0 <= ft < nt: hist[imu nt + (int) floor(ft)] += w; otherwise (a NaN too) outside_time += 1 -- such a ray
 *              has still entered the four planes above.  nt == 0: no time axis.
 * Output: double[nmu (4 + nt) + 10], ADDED into (zero it once; shards, beta-halves and several calls sum):
 *   [count | sum_w | sum_ws | sum_wt] (nmu each)  [hist (nmu x nt, [imu nt + j])]
 *   {ray_count, return, escape, lost, other, binned, outside_mu, outside_time, inbound, bad_g}                                    (counts as doubles)
 *   binned + outside_mu + inbound + bad_g == escape;   return + escape + lost + other == ray_count.
 * Refused (KR_EINVAL, before a device is touched): a null pointer, n < 0; nmu outside 1 ... 4096; nt < 0; nmu (4 + nt) > 2^24; dmu or (with nt > 0) dt
 * not positive or not finite; a non-finite mu0, t0, gamma or spin; dist < 0 or not finite; V = KR_V_PLUNGE (the kr_post_ form).
 * Out of scope: the absolute scale that joins the per-pixel response to this flux (it needs the emissivity table's normalisation); f32 records;
 * polarisation of the direct continuum; a histogram over phi_obs for an off-axis source; source_solid_angle's box test. */
typedef struct kr_observer_spec {
    kr_return_bins cls;      /* the classes; source_r = 0: no self-zone */
    double spin;             /* the a of the momentum: the spin the records were traced with */
    double mu0, dmu;         /* inclination bins: bin i holds mu0 + i dmu <= cos(theta_obs) < mu0 + (i + 1) dmu (bin 0 from mu0 - dmu) */
    double t0, dt;           /* time rows: row j holds t0 + j dt <= t_ref < t0 + (j + 1) dt */
    double dist;             /* radius of the reference sphere (the image plane's dist), or 0: t_ref = t */
    double gamma;            /* photon index of the weight */
    int32_t nmu, nt;         /* nt = 0: no time axis */
} kr_observer_spec;
#ifdef __cplusplus
static_assert(sizeof(kr_observer_spec) == 120, "kr_observer_spec is 120 bytes (raytrace_cpu_amd/capi.py ObserverSpec)");
#endif

/* The illumination map of the disc: the emissivity histogram of kr_emis_bins with the AZIMUTH of the landing point kept -- what a source that is
 * not on the axis (any kr_pointsource position, a kr_pointsource_vel_spec blob, a moving kr_healpix_source) does to the disc: the near side lit
 * first, brightest and most blueshifted, the far side behind the hole.  Per ray record (in the kr_post_ form after range_phi and redshift(V,
 * reverse, projradius, motion), phi as stored back):
 *   filter   that of kr_emis_bins: steps > 0, z = r cos(theta) < 1e-2, g > 0 with g = rays[].redshift, r >= rad.r_isco.  A ray that passes counts
 *            in disc_count, binned or not.
 *   radius   q = log(r / rad.r_min) / log(rad.dr) (rad.logbin) or (r - rad.r_min) / rad.dr; the ray goes on iff -1 < q < rad.nr, at ir = (int) q --
 *            the quotient and index rule of kr_emis_bins, the test made on q itself (a NaN fails; the band -1 < q <= 0 belongs to ir = 0).
 *   azimuth  nphi == 1: no phi test, ip = 0 (a NaN phi IS binned: the map is then the emissivity histogram).  Otherwise
 *              p = phi + phi_shift;   phi_w = p - 2 M_PI floor((p + M_PI) / (2 M_PI));   q_ph = (phi_w + M_PI) / dphi
 *            with dphi = 2 M_PI / nphi rounded once on the host (the wrap of kr_volume_map); the ray is binned iff q_ph >= 0 (a NaN or an
 *            infinite phi fails), at ip = min((int) q_ph, nphi - 1).  The wrap is floating arithmetic: a p one ulp below -M_PI wraps to just
 *            below M_PI, where q_ph rounds to nphi itself -- the last cell, hence the min; a p one ulp below M_PI has p + M_PI round up to 2 M_PI
 *            and wraps to one ulp below -M_PI, q_ph < 0: such a record is in no cell (it shows in disc_count - binned).
 *   binned   at cell c = ir nphi + ip, the per-ray terms of the emissivity histogram:
 *              count[c] += 1;  flux[c] += 1 / (rad.num_primary_rays g);  emis[c] += g^-rad.gamma;  sum_redshift[c] += g;  sum_time[c] += t;
 *            binned += 1.
 * Output: double[5 ncell + 2] with ncell = nr nphi = [count | flux | emis | sum_redshift | sum_time] (ncell each, [ir nphi + ip]), disc_count, binned;
 * counts are doubles.  ADDED into (zero it once; shards and several calls sum).  Summed over ip the five planes are those of
 * kr_reduce_emissivity_dev_f64 less the rays whose azimuth failed (disc_count - binned counts those and the rays outside the radial range).
 * phi_shift turns the map against the records: the metric is axisymmetric, so the trace of a source at phi_s = 0 serves a source at phi_s = delta
 * with phi_shift = +delta here (and -delta in a table that is applied to disc records).
 * Refused (KR_EINVAL, before a device is touched): a null pointer, n < 0, nr < 1, nphi < 1, nr nphi > 2^20, a non-finite phi_shift, V = KR_V_PLUNGE
 * (the kr_post_ form).  Out of scope: the plunging flow, records that ended on a surface (kr_reduce_emissivity_surface_dev_f64), f32 records, and
 * the passes other than the line and the response (kr_illum_table below) that could read such a map as a table. */
typedef struct kr_illum_bins {
    kr_emis_bins rad;        /* filter, radial edges, gamma, num_primary_rays: exactly the emissivity histogram's */
    double phi_shift;        /* added to the record's phi before the wrap */
    int32_t nphi, pad;       /* azimuthal cells of 2 pi / nphi from phi = -pi */
} kr_illum_bins;
#ifdef __cplusplus
static_assert(sizeof(kr_illum_bins) == 72, "kr_illum_bins is 72 bytes (raytrace_cpu_amd/capi.py IllumBins)");
#endif

/* An illumination map as an (r, phi) TABLE of the line and of the response: the emissivity and the source -> disc delay that a source which is not on
 * the axis gives every cell of the disc, read by the passes over the DISC records of an image plane (kr_post_line_illum_dev_f64 and the five entry
 * points beside it).  Everything is as the flat twin of the entry point states it for a radial table, except where the two values come from.  Per disc
 * record that passed the twin's filter, with r and the record's stored (wrapped) phi:
 *   radius   fi = log(r / r_min) / log(dr) (logbin) or (r - r_min) / dr; the record has a ring iff -1 < fi < nr, ir = (int) fi -- the truncated table
 *            index of kr_line_bins.
 *   azimuth  the wrap and the ip rule of kr_illum_bins on the record's phi: p = phi + phi_shift, phi_w, q_ph = (phi_w + M_PI) / dphi, a cell iff
 *            q_ph >= 0, ip = min((int) q_ph, nphi - 1); nphi == 1: ip = 0 and no phi test.
 *   values   emis = emis[ir nphi + ip];   tt = time ? time[ir nphi + ip] : 0.
 * A record without ir, with a q_ph that is not >= 0 (a NaN), or whose cell holds a non-finite emis or tt passed the filter (it counts in on_disc) and is
 * not used -- as the radial tables treat such a record.  The time expression keeps its operand order, (t + tt - t0) / dt.
 * phi_shift is the orbital phase: the metric is axisymmetric, so ONE source trace at phi_s = 0 (a map made with phi_shift = 0) serves the source at
 * every phase delta through phi_shift = -delta here.
 * Refused (KR_EINVAL, before a device is touched): what the twin refuses; a null table or a table without emis; nr < 1; nphi < 1; nr nphi > 2^20; a
 * non-finite r_min, dr or phi_shift; bins or a model that carry table_emis or table_time of their own; V = KR_V_PLUNGE.
 * Not covered: the continuum spectrum pass (it has no time axis), the hot spot, the Stokes passes, the surface passes, the plunging flow, f32. */
typedef struct kr_illum_table {
    double r_min, dr;        /* radial index: the truncated table index of kr_line_bins */
    double phi_shift;        /* the map's wrap and ip rule, on the DISC record's phi */
    const double* emis;      /* HOST, nr x nphi, [ir nphi + ip]; required */
    const double* time;      /* HOST, nr x nphi source -> disc delay, or NULL */
    int32_t nr, nphi, logbin, pad;
} kr_illum_table;
#ifdef __cplusplus
static_assert(sizeof(kr_illum_table) == 56, "kr_illum_table is 56 bytes (raytrace_cpu_amd/capi.py IllumTable)");
#endif

/* ---- runtime ---------------------------------------------------------------------------------- */
int         kr_abi_version(void);
const char* kr_last_error(void);
int         kr_device_count(void);                 /* <0: KR_ENODEVICE */
int         kr_set_device(int device);
int         kr_device_info(int* cu_count, int* clock_khz, int64_t* hbm_bytes, char* name, int name_len);
void        kr_params_default(kr_params* p, double spin);   /* Raytracer ctor defaults, raytracer.cpp:12-22 */
double      kr_kerr_horizon(double a);                      /* kerr_horizon(), src/include/kerr.h:14-20 */
double      kr_kerr_isco(double a, int sign);               /* kerr_isco(), kerr.h:23-32 (float-rounded A, B: sic) */
double      kr_disc_velocity(double r, double a, int sign); /* disc_velocity(), kerr.h:35-38 */
int64_t     kr_pointsource_count(const kr_pointsource* s, int32_t* n_cosalpha, int32_t* n_beta);   /* pointsource.cpp:12,16-17 */
int64_t     kr_imageplane_count(const kr_imageplane* s, int32_t* nx, int32_t* ny);                 /* imageplane.cpp:12-14 */
int64_t     kr_bundles_count(const kr_imageplane* s, int32_t* nx, int32_t* ny);                    /* imageplane_bundles.h:150-153: 5 * int(product of doubles) */
/* The transcendental values of the PointSource constructor (pointsource.cpp:38-46: alpha = acos(cosalpha0 + i dcosalpha), beta = beta0 + j dbeta;
 * raytracer.cpp:631-672: sin / cos of alpha and beta, sin / cos / tan of the source's polar angle pos[2]) computed on the HOST with the C library
 * the reference calls.  The device constructors (kr_pointsource_init*_dev_f64) read exactly these -- they upload them once per (device, grid), and
 * the copy stays while the device's table cache has room (freed only when no call holds it and the device has drained, or by kr_shutdown) -- so
 * k, h, Q of a device-built ray carry the reference constructor's bits.  Needs no GPU.
 * alpha_sincos: 2 * n_cosalpha doubles (sin, cos interleaved); beta_sincos: 2 * n_beta; pos_sin_cos_tan: 3.  Any of them may be NULL. */
int         kr_pointsource_tables(const kr_pointsource* s, double* alpha_sincos, double* beta_sincos, double* pos_sin_cos_tan);

/* ---- the hot path: Raytracer<T>::run_raytrace, both overloads (raytracer.cpp:63-127, 972-1034) --
 * Host-pointer forms stage through a private device buffer and return when rays[] is final.  *_dev forms take a device
 * pointer and a hipStream_t (NULL: the default stream): work is enqueued on that stream and, with stats == NULL, the call
 * returns before it has finished; nothing in the launch path waits for the device.  Every call draws its queue counters,
 * index list, events and second stream from a per-device pool of workspaces and gives them back when its last kernel
 * has finished, so any number of traces may be in flight on one device, from several streams or host threads
 * (multi-launch drivers -- one launch per source radius, one per tolerance -- overlap their long-ray tails that way). */
int kr_trace_f64(const kr_params* p, kr_ray_f64* rays, int64_t n, kr_stats* stats);
int kr_trace_f32(const kr_params* p, kr_ray_f32* rays, int64_t n, kr_stats* stats);
int kr_trace_dev_f64(const kr_params* p, void* d_rays, int64_t n, void* stream, kr_stats* stats);
int kr_trace_dev_f32(const kr_params* p, void* d_rays, int64_t n, void* stream, kr_stats* stats);
/* The same trace in two halves, for callers that want the counters of overlapping launches: kr_trace_async_* enqueues and
 * returns a ticket at once; kr_trace_wait blocks until THAT trace has finished, fills *stats (may be NULL) and retires the
 * ticket; kr_trace_release retires it without waiting.  Every ticket must go to exactly one of the two (at most 512 may be
 * outstanding per device).  kr_trace_dev_*(.., stats) == async + wait;  (.., NULL) == async + release. */
int kr_trace_async_f64(const kr_params* p, void* d_rays, int64_t n, void* stream, void** ticket);
int kr_trace_async_f32(const kr_params* p, void* d_rays, int64_t n, void* stream, void** ticket);
/* `count` traces at once (one per tolerance of a sweep, per source radius, ...), each with its own ray buffer.  When all of them use the
 * same kernel instances (same integrator, same kind of stop surface, same arithmetic flags; count <= 256, every n >= 4096) the batch is
 * MERGED: one classification per trace, then ONE strict side launch and ONE main launch over all traces (every wave serves one of the
 * traces' queues), on streams[0]; other streams wait for the batch at both ends, so whatever the caller enqueued on streams[i] before
 * the call is seen and whatever it enqueues afterwards sees trace i's result -- but a merged batch wants ONE stream for all its traces
 * (18 streams waiting on it cost the 18-point RK45 sweep 2.5-6 s instead of 0.41 s).  Otherwise the strict side
 * launches of all traces are enqueued before any main launch, each trace on its own stream.  Strict traces are split whatever their
 * size.  Same results and counters as `count` kr_trace_async_f64 calls, bit for bit (kernel_ms etc. then time the whole batch).
 * streams may be NULL (all on the default stream). */
int kr_trace_batch_async_f64(int32_t count, const kr_params* const* p, void* const* d_rays, const int64_t* n, void* const* streams, void** tickets);
int kr_trace_wait(void* ticket, kr_stats* stats);
/* kr_trace_wait on `count` tickets (a batch's, in any order).  per_ticket (optional): count records; total (optional): the counters summed
 * (rays_total, rays_traced, steps_total, rk45_*, rays_strict_side) and the LARGEST kernel_ms / strict_side_ms / main_ms / longest_ray_steps*.  Every ticket is
 * released, also when one of them fails (the first error code is returned). */
int kr_trace_wait_many(int32_t count, void* const* tickets, kr_stats* per_ticket, kr_stats* total);
int kr_trace_release(void* ticket);
/* Progress of a trace in flight (run_raytrace's show_progress, raytracer.cpp:84-85, :107-115: a counter of rays whose loop iteration has STARTED).
 * kr_trace_poll: how many rays the trace behind `ticket` has taken off its work queue so far and whether it has finished; it neither waits nor
 * retires the ticket (an 8-byte DMA read of the queue head on a stream of the library's own: it completes while the trace kernels hold every SIMD).
 * kr_trace_progress_*: kr_trace_* (host pointers) which, while the trace runs, polls every 20 ms on the calling thread and calls
 * fn(rays_started rounded down to a multiple of `every`, n, user) each time a new multiple has been passed.  every <= 0 or fn == NULL: no calls. */
typedef void (*kr_progress_fn)(int64_t rays_started, int64_t rays_total, void* user);
int kr_trace_poll(void* ticket, int64_t* rays_started, int32_t* finished);
int kr_trace_progress_f64(const kr_params* p, kr_ray_f64* rays, int64_t n, kr_stats* stats, int64_t every, kr_progress_fn fn, void* user);
int kr_trace_progress_f32(const kr_params* p, kr_ray_f32* rays, int64_t n, kr_stats* stats, int64_t every, kr_progress_fn fn, void* user);

/* ---- per-step ray paths: run_raytrace(method, theta_max, r_max, show_progress, outfile, write_step, write_rmax, write_rmin, write_cartesian),
 * the serial branch raytracer.cpp:86-100, for Integrator::Euler and Integrator::RK4 in double precision with the strict arithmetic (flags = 0:
 * a recorded ray takes exactly the steps, and ends with exactly the record, of kr_trace_dev_f64 with flags = 0).
 * Write rule (raytracer.cpp:293-312 Euler, :923-942 and :1209-1228 RK4): with `steps` this call's own counter, incremented at the top of every
 * iteration, a row {t, r, theta, phi} is written after the state update of an iteration when steps % write_step == 0 and
 * (write_rmax < 0 || r < write_rmax) && (write_rmin < 0 || r > write_rmin).  A theta-flip iteration (`continue`), one that ends on r <= horizon and one
 * that ends on dest->reached() write nothing; an iteration whose update makes the loop condition false does.  When a row is due, the window
 * test fails and this ray has written a row before, the ray stops there (:308-311) and its record is what the epilogue makes of that state.
 * Rays skipped by the skip rule (steps < 0 || steps >= steplim, :91-92) have no rows and traced = 0: a text writer puts the reference's two
 * blank lines (:99) after traced rays only.
 * Layout: ray i owns rows[offsets[i] .. offsets[i + 1]), a row is four doubles; always Boyer-Lindquist -- write_cartesian is applied by the host-side
 * writers with cartesian() (src/include/kerr.h:41-48) and the C library, O(rows) next to formatting them.
 * Two passes: kr_trace_paths_count_dev_f64 integrates every ray, stores the row counts, scans them into d_offsets[0 .. n] and returns
 * *total_rows = offsets[n]; d_rays is NOT modified.  It SYNCHRONISES `stream` (the total goes to the host).  The caller allocates d_rows and calls
 * kr_trace_paths_record_dev_f64 with the same params, spec and rays: it integrates again, stores the rows and the final ray records (as a trace
 * does) and fills *stats (may be NULL: rays_total, rays_traced, steps_total, longest_ray_steps, kernel_ms).  It SYNCHRONISES `stream` too: it returns
 * KR_EINVAL if any ray wrote another number of rows than its slab holds (nothing is ever stored outside a ray's slab or beyond total_rows).
 * Refused with KR_EINVAL before any device work: null pointers, n < 0, write_step <= 0, NaN window bounds, KR_FLAG_FAST_MATH / KR_FLAG_HYBRID (paths carry
 * the reference's arithmetic), KR_RK45, Euler with a destination stop kind (raytracer.cpp:983), d_rows not 32-byte aligned; total_rows < offsets[n] once
 * the device has been asked for it.  Without a device: KR_ENODEVICE.
 * RK45 is deliberately left out: its step is one TRIAL per wave iteration with retries, a replay mode and extrapolation (kr_rk45.hpp), and
 * none of the reference's programs records it (trace_rays.cpp:71, trace_rays_imageplane.cpp:61 hard-wire Euler).
 * kr_trace_paths_f64: host pointers; stages rays[], runs both passes and returns with rays[], offsets[0 .. n], traced[0 .. n) (may be NULL) filled and
 * *rows pointing at 4 * *total_rows doubles of page-locked memory that the CALLER frees with kr_host_free. */
int kr_trace_paths_count_dev_f64(const kr_params* p, const kr_path_spec* w, const void* d_rays, int64_t n, void* d_offsets /* int64[n + 1] */,
                                 void* d_traced /* uint8[n] or NULL */, int64_t* total_rows, void* stream);
int kr_trace_paths_record_dev_f64(const kr_params* p, const kr_path_spec* w, void* d_rays, int64_t n, const void* d_offsets, void* d_rows /* double[total_rows][4] */,
                                  int64_t total_rows, void* stream, kr_stats* stats);
int kr_trace_paths_f64(const kr_params* p, const kr_path_spec* w, kr_ray_f64* rays, int64_t n, int64_t* offsets /* n + 1 */, uint8_t* traced /* n or NULL */,
                       double** rows, int64_t* total_rows, kr_stats* stats);

/* ---- volume illumination maps: Mapper::map_ray (src/mapper/mapper.cpp:110-281) restated against the loop above -- every ray is binned into the
 * (r, theta, phi) grid of a kr_volume_map AS IT STEPS, with its arrival time and energy shift.  Euler and RK4, double precision, strict arithmetic.
 * Rows: a ray produces a row {t, r, theta, phi} after the state update of every iteration that is neither a theta flip nor one that ended on
 * r <= horizon or on dest->reached(): exactly the rows kr_trace_paths_* writes with write_step = 1 and an open window (an iteration whose update
 * makes the loop condition false has a row, the start point has none).
 * Cell: q_r = logbin ? log(r / r_min) / log(dr) : (r - r_min) / dr;  q_th = theta / dtheta;  q_ph = (phi_w + M_PI) / dphi with
 * phi_w = phi - 2 M_PI floor((phi + M_PI) / (2 M_PI)); with nphi == 1 there is no phi test and no wrap, iphi = 0 (the axisymmetric map).  The row is
 * in the grid iff 0 <= q < n on every axis, decided on q itself (a NaN or infinite q is outside, and no error: kr_emis_bins' convention); its cell
 * is ((int) q_r * ntheta + (int) q_th) * nphi + (int) q_ph (Array3D's layout).  Apart from the log each is a single IEEE operation.
 * Deposit: mode 0 (passage) -- every ray keeps last_cell, -1 when it starts; a row deposits iff it is in the grid and its cell differs from
 * last_cell; last_cell then becomes the row's cell, or -1 for a row outside the grid, whether or not g passed.  mode 1 -- every row in the grid deposits.
 * A due deposit evaluates g = ray_redshift(V, reverse, projradius, r, theta, phi, k, h, Q, rdot_sign, thetadot_sign, emit, motion) (raytracer.cpp:480-553,
 * as kr_redshift_dev_f64 does) at the row, emit from the ray's record; g > 0 and finite: count[cell] += 1, time[cell] += t, redshift[cell] += g;
 * otherwise only bad_g moves.
 * Departures from mapper.cpp, both deliberate: its range test `ir > 0 && ...` (:247) drops cell 0 of every axis -- here cell 0 is a cell; it never
 * assigns last_ir / last_itheta / last_iphi, so it deposits at every step (mode 1) where the consumers of the map expect mode 0.  vel_mode 1 / 2 are
 * not offered.
 * d_map: double[3 ncell + 4], ncell = nr ntheta nphi: [count | time | redshift | rows, in_grid, deposits, bad_g]; counts are whole-numbered doubles,
 * rows == offsets[n] of the write_step = 1 recording, deposits == the sum of count.
 * kr_trace_volume_dev_f64 integrates every ray as kr_trace_dev_f64 with flags = 0 does -- d_rays ends with that trace's records, bit for bit -- and
 * ADDS into d_map, so sources, shards and batches sum into one map (calls into one map from several streams may overlap: every addition is atomic).
 * It fills *stats (may be NULL: rays_total, rays_traced, steps_total, longest_ray_steps, kernel_ms: the map launch and the kernel that adds its
 * tallies) and SYNCHRONISES `stream` before it returns (the launch's counters come back to the host).
 * n == 0 leaves d_map untouched.  kr_trace_volume_f64: host pointers; stages rays[], and map[0 .. 3 ncell + 4) is OVERWRITTEN.
 * Refused with KR_EINVAL before any device work: null pointers, n < 0, nr / ntheta / nphi < 1, ncell > 2^27, dr / dtheta / dphi not finite or <= 0,
 * logbin with dr <= 1 or r_min <= 0, an unknown mode or motion, and what kr_trace_paths_* refuses of a kr_params: KR_FLAG_FAST_MATH / KR_FLAG_HYBRID,
 * KR_RK45, Euler with a destination stop kind.  Without a device: KR_ENODEVICE. */
int kr_trace_volume_dev_f64(const kr_params* p, const kr_volume_map* m, void* d_rays, int64_t n, void* d_map /* double[3 ncell + 4] */, void* stream, kr_stats* stats);
int kr_trace_volume_f64(const kr_params* p, const kr_volume_map* m, kr_ray_f64* rays, int64_t n, double* map /* 3 ncell + 4 */, kr_stats* stats);

/* ---- observing a volume map: SourceTracer::propagate_source (src/source_tracer/source_tracer.cpp:102-310) restated against the loop above -- camera
 * rays are marched back through the emitting volume and gather, AS THEY STEP, the emissivity of the cells they cross into an energy spectrum, an
 * energy-time response and a per-ray total.  Euler and RK4, double precision, strict arithmetic.
 * Rows: those of kr_trace_volume_*: the state after the update of every iteration that is neither a theta flip nor one that ended on r <= horizon or
 * on dest->reached().
 * Step displacement: the position before the step is the previous row, or the ray's initial record for its first row (a flip iteration moves nothing,
 * so this is the ray's state as the iteration begins); dr, dtheta, dphi = row - before.
 * Cell: as in the volume map -- the same kr_volume_map and the same quotients; the phi used is the ray's own (an ImagePlane ray in the mirrored spin
 * carries the physical phi of the photon it reverses: no mirroring).  m->mode is validated and otherwise unused (this is a line integral);
 * V, reverse, projradius, motion describe the emitter's frame as they do for the map.
 * Inputs per cell, device arrays of ncell doubles: emis, the volume emissivity j; kappa, the absorption per unit proper length (NULL: optically thin);
 * delay, the time from the flash to the cell (NULL: 0).
 * Bins: kr_observe_bins.  q_e = logbin_en ? log(E / en0) / log(den) : (E - en0) / den;  q_t = (T - t0) / dt.  Range tests are decided on q itself
 * (a NaN or infinite q is outside).
 * Per row, in this order:
 *  1. cell < 0: stop.  Otherwise ++in_grid.
 *  2. j = emis[cell], kap = kappa ? kappa[cell] : 0.  !(j > 0) && !(kap > 0): stop.  Otherwise ++lit.
 *  3. l = sqrt((Sigma / Delta) dr^2 + Sigma dtheta^2 + (A sin^2 theta / Sigma) dphi^2) at the row, Sigma = r^2 + a^2 cos^2 theta,
 *     Delta = r^2 - 2 r + a^2, A = (r^2 + a^2)^2 - a^2 Delta sin^2 theta.  !(l > 0 && l < inf && |dphi| < pi / 2): ++degenerate, stop (the polar
 *     reflection adds pi to phi: that row is dropped here).
 *  4. j > 0: z = ray_redshift(...) at the row as kr_trace_volume_* evaluates it (the lane's signs, the ray's emit).  !(z > 0 && z < inf): ++bad_g.
 *     Otherwise E = 1 / z, w = j l E E E, times exp(-tau) when kappa != NULL; image_ray += w, ++contributions; if 0 <= q_e < nen:
 *     spectrum[(int) q_e] += w, hits[(int) q_e] += 1, and when nt > 0, T = t_row + (delay ? delay[cell] : 0), if 0 <= q_t < nt:
 *     response[(int) q_e * nt + (int) q_t] += w.
 *  5. tau += l kap.  tau is per ray and 0 when the ray starts.
 * Departures from source_tracer.cpp, all deliberate: the square root in l (its `len`, :234, is a squared length); ONE grey tau per ray where it keeps
 * absorb[ray][ien] per observed-energy bin; the time bin uses the bin width, not the step's dt that shadows it (:208, :263); the region and the
 * emissivity come from the grid, not the hard-wired shell (:232, :247-258); no per-ray spectra (n x nen doubles is not a product) -- the per-ray total
 * replaces them.
 * d_out: double[2 nen + nen nt + 6]: [spectrum | hits | response | rows, in_grid, lit, contributions, bad_g, degenerate]; counts are whole-numbered
 * doubles.  kr_trace_observe_dev_f64 integrates every ray as kr_trace_dev_f64 with flags = 0 does -- d_rays ends with that trace's records, bit for
 * bit -- and ADDS into d_out, so shards and several planes sum into one result (every addition is atomic).  d_image: double[n] or NULL, OVERWRITTEN:
 * the ray's total, 0 for a ray the skip rule passed over.  It fills *stats (may be NULL) and SYNCHRONISES `stream` before it returns, as
 * kr_trace_volume_dev_f64 does.  n == 0 leaves d_out untouched.  kr_trace_observe_f64: host pointers; stages everything, out[] is OVERWRITTEN.
 * Refused with KR_EINVAL before any device work: everything kr_trace_volume_* refuses; null b, emis, out or (n > 0) rays; nen < 1, nt < 0,
 * 2 nen + nen nt > 2^27; den not finite or <= 0; logbin_en with den <= 1 or en0 <= 0; nt > 0 with dt not finite or <= 0; a non-finite en0 or t0.
 * Without a device: KR_ENODEVICE. */
int kr_trace_observe_dev_f64(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const void* d_emis, const void* d_kappa, const void* d_delay,
                             void* d_rays, int64_t n, void* d_out /* double[2 nen + nen nt + 6] */, void* d_image /* double[n] or NULL */, void* stream, kr_stats* stats);
int kr_trace_observe_f64(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const double* emis, const double* kappa, const double* delay,
                         kr_ray_f64* rays, int64_t n, double* out /* 2 nen + nen nt + 6 */, double* image /* n or NULL */, kr_stats* stats);

/* ---- equatorial crossings: where and when a ray meets the plane theta = pi / 2, EVERY time it does, with the energy shift of an emitter on the plane
 * there.  Crossing number m of a camera ray is the image of order m of an equatorial disc: the direct image (0), the underside seen over the top of
 * the hole (1), the photon ring (>= 2).  Euler and RK4, double precision, strict arithmetic, on the loop above.
 * Crossing: an iteration crossed iff it moved the trace's own counter rays[i].equatorial_crossings -- with theta before and after the state update
 * (before the reflection at the poles), (before < M_PI/2 && after >= M_PI/2) || (before > M_PI/2 && after <= M_PI/2).  A theta-flip iteration moves
 * nothing and never crosses; an iteration that ends on r <= horizon or on dest->reached() counts like any other (the disc of a KR_STOP_DISC_ISCO trace
 * is met in exactly such an iteration).
 * Where: with (t0, r0, theta0, phi0) the ray's state before the iteration and (t1, r1, theta1, phi1) after it (after the reflection at the poles),
 *     f   = (M_PI/2 - theta0) / (theta1 - theta0)
 *     r_c = r0 + f (r1 - r0)     phi_c = phi0 + f (phi1 - phi0)     t_c = t0 + f (t1 - t0)
 * each a single IEEE operation in this association, no contraction.
 * g = ray_redshift(V, reverse, projradius, r_c, M_PI/2, ., k, h, Q, rdot_sign, thetadot_sign, emit, motion) (raytracer.cpp:480-553, as kr_redshift_dev_f64
 * does) with the ray's k, h, Q, the signs the ray has after that iteration and emit from the ray's record.
 * Storing: every ray counts its crossings in this call, `seen`, from 0.  A crossing made with seen < M = max_crossings is stored as
 * d_rows[(i M + seen) 4 ..] = {r_c, phi_c, t_c, g}; g is stored as computed (NaN and g <= 0 included: consumers filter).  Then ++seen, always.  Rows
 * m >= min(seen, M) of a ray are NOT written (fill d_rows beforehand to tell them apart); nothing is ever stored outside a ray's slab of M rows.
 * d_seen[i] = seen, 0 for a ray the skip rule (steps < 0 || steps >= steplim) passed over: for every traced ray the increase of
 * rays[i].equatorial_crossings in this call (with stop_when_full, at most M).
 * stop_when_full: the iteration that makes a ray's M-th crossing is its last: the ray ends with that iteration's state and its record is what the
 * epilogue makes of it (the mechanism of a path recording that leaves its window): no status bit of its own -- whatever ERGO / NEG_ENERGY flags its steps
 * raised, HORIZON or DEST if that iteration ended on one anyway, STEPLIM / RLIM / DEST only if that state meets the epilogue's tests; a ray cut short in
 * mid-flight has status 0 and steps > 0.  It removes the rays that whirl at the photon sphere for 1e6 steps and more, each half orbit a crossing.
 * Every ray the recorder did not end -- every ray, without stop_when_full -- finishes with the record of kr_trace_dev_f64 with flags = 0, bit for bit.
 * kr_trace_crossings_dev_f64 fills *stats (may be NULL: rays_total, rays_traced, steps_total, longest_ray_steps, kernel_ms) and SYNCHRONISES `stream`
 * before it returns (the launch's counters come back to the host).  No atomics: a ray's rows and d_seen[i] are written by the lane that holds it.
 * n == 0 touches nothing.  kr_trace_crossings_f64: host pointers; stages rays[], rows[] and seen[]; rows[] is copied to the device first and back as
 * it is there afterwards, so rows that were not written keep the caller's values.
 * Refused with KR_EINVAL before any device work: null pointers, n < 0, max_crossings outside 1..16, an unknown motion, d_rows not 32-byte aligned (a
 * row is two 16-byte stores), and what kr_trace_paths_* refuses of a kr_params: KR_FLAG_FAST_MATH / KR_FLAG_HYBRID, KR_RK45, Euler with a destination
 * stop kind.  Without a device: KR_ENODEVICE.
 * kr_reduce_crossing_image_dev_f64: the image of ONE order, one work-item per ray.  order >= 0 takes crossing `order` of every ray with
 * order < min(seen, M); order = -1 (the opaque disc) takes a ray's first stored crossing with r_isco <= r_c < r_disc (a NaN fails the test; g plays
 * no part in the choice).  The chosen crossing is accumulated as kr_reduce_image_dev_f64 accumulates a record with steps = 1, r = r_c, theta = M_PI/2,
 * phi = range_phi(phi_c; lo, hi), t = t_c, redshift = g and the alpha, beta of d_rays[i]: the same tests (g > 0, the radial range, the pixel) and the same
 * sums.  It ADDS into d_planes, double[7 img_nx img_ny + 1] in that reducer's layout, so whatever reads a direct image's planes reads an order's
 * (kr_line_from_image_dev_f64 on them gives the order's line profile); it does not wait for `stream`.  Refused with KR_EINVAL: null pointers (d_rays,
 * d_rows, d_seen only when n > 0), n < 0, a non-positive image size, max_crossings outside 1..16, order outside [-1, max_crossings). */
int kr_trace_crossings_dev_f64(const kr_params* p, const kr_crossing_spec* spec, void* d_rays, int64_t n, void* d_rows /* double[n][M][4] */,
                               void* d_seen /* int32[n] */, void* stream, kr_stats* stats);
int kr_trace_crossings_f64(const kr_params* p, const kr_crossing_spec* spec, kr_ray_f64* rays, int64_t n, double* rows /* n M 4 */, int32_t* seen /* n */,
                           kr_stats* stats);
int kr_reduce_crossing_image_dev_f64(const kr_image_bins* b, int32_t max_crossings, int32_t order, double lo, double hi, const void* d_rays, const void* d_rows,
                                     const void* d_seen, int64_t n, void* d_planes, void* stream);

/* ---- the disc flow "Keplerian, plunging inside the ISCO" -------------------------------------------------------------------------------------
 * V == KR_V_PLUNGE with motion = 0 selects it in the passes that take V (V == -1 stays the Keplerian observer at every radius).  With the metric's
 * a = reverse ? -spin : spin and r_ms = kr_kerr_isco(a, +1) -- the float-rounded ISCO the programs use as the disc's inner edge:
 *   r >= r_ms   the observer, frame and every output bit of V = -1
 *   r <  r_ms   the gas on the equatorial geodesic that left the circular orbit at r_ms with its energy and angular momentum; u = 1 / r_ms,
 *               Delta = r r - 2 r + a a, every square root a double one (the host area code, host/include/disc.h, keeps the reference's sqrtf):
 *                 E_ms = (1 - 2u + a u sqrt(u)) / sqrt(1 - 3u + 2 a u sqrt(u))
 *                 L_ms = (1 + a a u u - 2 a u sqrt(u)) / sqrt(u (1 - 3u + 2 a u sqrt(u)))
 *                 u^t  = ((r r + a a + 2 a a / r) E_ms - 2 a L_ms / r) / Delta
 *                 u^phi = (2 a E_ms / r + (1 - 2 / r) L_ms) / Delta
 *                 u^r  = -sqrt(max(0, E_ms^2 - 1 + 2 / r + (a a (E_ms^2 - 1) - L_ms^2) / (r r) + 2 (L_ms - a E_ms)^2 / (r r r))),  u^theta = 0
 *               r_ms, E_ms, L_ms are computed once per launch on the host.  The received energy is the sum over all sixteen (i, j) of g_ij u^i p^j in the
 *               metric at the record's own (r, theta) (the disc filter admits |z| < 1e-2).  Frame: e_t = u; e2 = (0, 0, 1 / sqrt(rhosq), 0) as for V = -1,
 *               so mu = |P_th| / E changes only through E; e3 (r-like) and e1 (phi-like) by Gram-Schmidt against the metric, seeds d/dr then d/dphi,
 *               projections removed before any leg is normalised (v -= (g(seed, e_j) / g(e_j, e_j)) e_j, j in order), each leg divided by
 *               sqrt(|g(e, e)|) and oriented e3^r > 0, e1^phi > 0 (host/include/gramschmidt_basis.h).  Bad-angle keeps its definition.
 * Accepted (f64, motion = 0, both reverse values): kr_redshift_f64 / _dev_f64, kr_angles_f64 / _dev_f64, kr_post_image_dev_f64, kr_post_emissivity_dev_f64,
 * kr_post_emissivity_mu_dev_f64, kr_post_line_dev_f64, kr_post_line_limb_dev_f64, kr_post_spectrum_dev_f64, kr_post_response_dev_f64.  The inner edge of
 * what is binned stays the r_isco field of the bins or model: a caller who wants the plunging region sets it to the inner radius of choice.
 * Refused with KR_EINVAL (the message names the function) before anything is launched: the f32 passes, motion = 1, kr_redshift_start_*, kr_post_hotspot_*
 * (its shear law is Keplerian), the three polarisation entry points (Walker-Penrose writes its own legs), the return map and its batch, the HEALPix map,
 * kr_post_angdist_*, the V of kr_volume_map and kr_crossing_spec, and every ray-source constructor.  Out of scope: polarisation, a hot spot inside the
 * ISCO, a plunge radius other than the ISCO, gas off the equatorial plane (the thick disc's surface passes keep V = -1). */
#define KR_V_PLUNGE (-2.0)
/* r_ms, E_ms, L_ms of the flow for the metric's a (needs no GPU); KR_EINVAL for a null pointer, |a| > 1 or NaN */
int kr_plunge_flow(double a, double* r_ms, double* E_ms, double* L_ms);
/* the flow's four-velocity (u^t, u^r, u^theta, u^phi) on the equatorial plane at r: the geodesic above for r < r_ms, the circular orbit's
 * (Omega = 1 / (a + r sqrt(r))) for r >= r_ms (needs no GPU); KR_EINVAL as above, and for r that is not finite or not outside the horizon */
int kr_plunge_velocity(double a, double r, double u[4]);

/* ---- O(N) passes either side of it ----------------------------------------------------------- */
/* Raytracer<T>::redshift_start(V, reverse, projradius)  raytracer.cpp:342-417 */
int kr_redshift_start_f64(double spin, double V, int reverse, int projradius, kr_ray_f64* rays, int64_t n);
int kr_redshift_start_dev_f64(double spin, double V, int reverse, int projradius, void* d_rays, int64_t n, void* stream);
/* Raytracer<T>::redshift(V, reverse, projradius, motion)  raytracer.cpp:420-447, 480-553 */
int kr_redshift_f64(double spin, double V, int reverse, int projradius, int motion, kr_ray_f64* rays, int64_t n);
int kr_redshift_dev_f64(double spin, double V, int reverse, int projradius, int motion, void* d_rays, int64_t n, void* stream);
/* Raytracer<T>::redshift(RayDestination*, reverse, ...) with the default four_velocity()
 * (raytracer.cpp:450-477, 556-600; ray_destination.h:59-78: every concrete class keeps velocity() = -1) */
int kr_redshift_dest_f64(double spin, int reverse, kr_ray_f64* rays, int64_t n);
int kr_redshift_dest_dev_f64(double spin, int reverse, void* d_rays, int64_t n, void* stream);
/* Raytracer<T>::range_phi(min, max)  raytracer.cpp:603-622 */
int kr_range_phi_f64(double lo, double hi, kr_ray_f64* rays, int64_t n);
int kr_range_phi_dev_f64(double lo, double hi, void* d_rays, int64_t n, void* stream);
/* Raytracer<T>::calculate_momentum()  raytracer.cpp:704-753 */
int kr_calculate_momentum_f64(double spin, kr_ray_f64* rays, int64_t n);
int kr_calculate_momentum_dev_f64(double spin, void* d_rays, int64_t n, void* stream);
/* The same five passes for Raytracer<float>: kr_ray_f32 records, float arithmetic throughout (the reference's float instantiation of the
 * same source lines; spin, V, lo, hi are float values carried in doubles).  Host-pointer forms copy the whole 84-byte record back. */
int kr_redshift_start_f32(double spin, double V, int reverse, int projradius, kr_ray_f32* rays, int64_t n);
int kr_redshift_start_dev_f32(double spin, double V, int reverse, int projradius, void* d_rays, int64_t n, void* stream);
int kr_redshift_f32(double spin, double V, int reverse, int projradius, int motion, kr_ray_f32* rays, int64_t n);
int kr_redshift_dev_f32(double spin, double V, int reverse, int projradius, int motion, void* d_rays, int64_t n, void* stream);
int kr_redshift_dest_f32(double spin, int reverse, kr_ray_f32* rays, int64_t n);
int kr_redshift_dest_dev_f32(double spin, int reverse, void* d_rays, int64_t n, void* stream);
int kr_range_phi_f32(double lo, double hi, kr_ray_f32* rays, int64_t n);
int kr_range_phi_dev_f32(double lo, double hi, void* d_rays, int64_t n, void* stream);
int kr_calculate_momentum_f32(double spin, kr_ray_f32* rays, int64_t n);
int kr_calculate_momentum_dev_f32(double spin, void* d_rays, int64_t n, void* stream);

/* ---- ray sources: PointSource / ImagePlane ctors (pointsource.cpp:11-64, imageplane.cpp:11-121) -- */
int kr_pointsource_init_f64(const kr_pointsource* s, kr_ray_f64* rays, int64_t n);
int kr_pointsource_init_dev_f64(const kr_pointsource* s, void* d_rays, int64_t n, void* stream);
int kr_imageplane_init_f64(const kr_imageplane* s, kr_ray_f64* rays, int64_t n);
int kr_imageplane_init_dev_f64(const kr_imageplane* s, void* d_rays, int64_t n, void* stream);
/* shard forms of the two ctors: slot k of d_rays receives ray (first + k*stride) of the source's own array, k < count.
 * Rank r of R uses first = r, stride = R: ray-cyclic sharding, nothing else has to be exchanged before the reducers. */
int kr_pointsource_init_strided_dev_f64(const kr_pointsource* s, int64_t first, int64_t stride, void* d_rays, int64_t count, void* stream);
int kr_imageplane_init_strided_dev_f64(const kr_imageplane* s, int64_t first, int64_t stride, void* d_rays, int64_t count, void* stream);

/* ---- fused ends of the emissivity pipeline (device-resident callers): the same per-ray arithmetic as the separate passes, one
 * pass over the records instead of two / three.  kr_pointsource_init_emit = PointSource ctor + redshift_start(V, reverse,
 * projradius) (pointsource.cpp:11-64 + raytracer.cpp:342-417), strided like kr_pointsource_init_strided_dev_f64;
 * kr_post_emissivity = range_phi(lo, hi) + redshift(V, reverse, projradius, motion) + the histogram of kr_reduce_emissivity_dev_f64
 * (raytracer.cpp:603-622, :420-553, emissivity.cpp:96-126); rays[] ends up exactly as after the separate calls. */
int kr_pointsource_init_emit_dev_f64(const kr_pointsource* s, int64_t first, int64_t stride, double V, int reverse, int projradius, void* d_rays, int64_t count,
                                     void* stream);
/* `count` sources at once -- the multi-radius drivers (disc_source_photonfrac_r.cpp:74-92: one PointSource per radius): what `count` calls of
 * kr_pointsource_init_emit_dev_f64(&s[i], 0, 1, V ? V[i] : s[i].V, reverse, projradius, d_rays[i], n[i], stream) write, bit for bit, in
 * ceil(count / 24) kernel launches instead of `count` (a hundred launches of 1e6 rays each reach a third of the store bandwidth of one large one).
 * s, V (may be NULL), d_rays and n are HOST arrays of `count` entries, read before the call returns. */
int kr_pointsource_init_emit_batch_dev_f64(int32_t count, const kr_pointsource* s, const double* V, int reverse, int projradius, void* const* d_rays, const int64_t* n,
                                           void* stream);
/* the same for the image pipeline: ImagePlane ctor + redshift_start(V, reverse, projradius) (imageplane.cpp:11-121; the negated spin
 * of the ImagePlane is applied inside), and redshift(V, reverse, projradius, motion) + range_phi(lo, hi) + the seven planes of
 * kr_reduce_image_dev_f64 (imageplane_disc_image.cpp:117-161; `spin` as stored by the Raytracer, i.e. negated) */
int kr_imageplane_init_emit_dev_f64(const kr_imageplane* s, int64_t first, int64_t stride, double V, int reverse, int projradius, void* d_rays, int64_t count,
                                    void* stream);
/* the same ctor for shards made of RUNS of rays: slot k receives source ray first + (k / run) * stride + k % run.  With run = (ray columns
 * per pixel column) * ny, stride = R * run and first = r * run, rank r of R owns whole pixel columns r, r + R, ... of the image: the ranks'
 * image planes are then disjoint and are GATHERED, not summed (bench.py --image-exchange gather).  run = 1 is the plain strided form. */
int kr_imageplane_init_emit_runs_dev_f64(const kr_imageplane* s, int64_t first, int64_t stride, int64_t run, double V, int reverse, int projradius, void* d_rays,
                                         int64_t count, void* stream);
int kr_post_image_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_image_bins* b, void* d_rays, int64_t n,
                          void* d_planes, void* stream);
int kr_post_emissivity_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_emis_bins* b, void* d_rays, int64_t n,
                               void* d_hist, void* stream);

/* ---- reducers of the two target apps --------------------------------------------------------- */
/* emissivity.cpp:96-126.  Outputs (length nr each): count, flux, emis, sum_redshift, sum_time -- the raw
 * accumulators BEFORE the divisions of emissivity.cpp:128-134; *disc_count = rays passing the filter. */
int kr_reduce_emissivity_f64(const kr_emis_bins* b, const kr_ray_f64* rays, int64_t n,
                             int64_t* count, double* flux, double* emis, double* sum_redshift, double* sum_time,
                             int64_t* disc_count);
/* d_hist: device buffer of nr*5+1 doubles laid out [count | flux | emis | sum_redshift | sum_time | disc_count];
 * counts are held as doubles (exact below 2^53).  The call ADDS into d_hist (zero it first). */
int kr_reduce_emissivity_dev_f64(const kr_emis_bins* b, const void* d_rays, int64_t n, void* d_hist, void* stream);
/* imageplane_disc_image.cpp:122-161.  Seven planes of img_nx*img_ny, [ix*img_ny + iy] like Array2D:
 * nrays(int32), flux, r, phi, enshift, time, emis -- raw sums BEFORE the divisions of :165-174. */
int kr_reduce_image_f64(const kr_image_bins* b, const kr_ray_f64* rays, int64_t n,
                        int32_t* nrays, double* flux, double* r, double* phi, double* enshift, double* time,
                        double* emis, int64_t* disc_count);
/* d_planes: device buffer of 7*img_nx*img_ny+1 doubles [nrays | flux | r | phi | enshift | time | emis | disc_count],
 * nrays held as doubles.  ADDS into d_planes. */
int kr_reduce_image_dev_f64(const kr_image_bins* b, const void* d_rays, int64_t n, void* d_planes, void* stream);

/* ---- the same two reducers for rays that LANDED ON A SURFACE (a RayDestination stop such as KR_STOP_THICKDISC).  The reducers above hard-wire
 * z = r cos(theta) < 1e-2 and bin by r; these take the stop itself for the filter and the cylindrical radius of the landing point for the bins.
 * Per ray record, with rho = r sin(theta), z = r cos(theta) (the strict trace's sin / cos) and g = rays[].redshift:
 *   filter   steps > 0, status & KR_STATUS_DEST, g > 0 (a NaN fails)
 * Emissivity:  further rho >= b.r_isco (a NaN fails).  A ray that passes counts in disc_count, in upper if z > 0 and in lower if z < 0.  It is
 *   binned iff -1 < q < nr with q = log(rho / r_min) / log(dr) (logbin) or (rho - r_min) / dr -- the quotient and index rule of kr_emis_bins, the
 *   test made on q itself -- at ir = (int) q:  count += 1, flux += 1 / (num_primary_rays g), emis += g^-gamma, sum_redshift += g, sum_time += t,
 *   sum_z += z;  binned += 1.  sum_z / count is the mean landing height of a bin (about zero for a symmetric illumination: upper / lower tell).
 *   d_hist: double[6 nr + 4] = [count | flux | emis | sum_redshift | sum_time | sum_z](nr each) + disc_count, binned, upper, lower; counts are
 *   doubles.  ADDS into d_hist (zero it first).
 * Image:  further b.r_isco <= rho < b.r_disc, then the pixel rule of kr_image_bins unchanged.  d_planes: double[7 img_nx img_ny + 1], the layout of
 *   kr_reduce_image_dev_f64, with the powerlaw3 emissivity evaluated at rho and the radius plane holding rho.  ADDS into d_planes.
 * kr_post_*_surface = range_phi(lo, hi) + redshift(V = -1, reverse, projradius = 1, motion = 0) -- the Keplerian observer at the cylindrical radius,
 * 1 / (a + rho sqrt(rho)), `spin` as stored by the Raytracer -- + the reducer in one pass; rays[] ends up exactly as after the separate calls.
 * Refused with KR_EINVAL: null bins or result buffer, null d_rays with n > 0, nr <= 0, a non-positive image size. */
int kr_reduce_emissivity_surface_dev_f64(const kr_emis_bins* b, const void* d_rays, int64_t n, void* d_hist, void* stream);
int kr_post_emissivity_surface_dev_f64(double spin, int reverse, double lo, double hi, const kr_emis_bins* b, void* d_rays, int64_t n, void* d_hist, void* stream);
int kr_reduce_image_surface_dev_f64(const kr_image_bins* b, const void* d_rays, int64_t n, void* d_planes, void* stream);
int kr_post_image_surface_dev_f64(double spin, int reverse, double lo, double hi, const kr_image_bins* b, void* d_rays, int64_t n, void* d_planes, void* stream);

/* disc_source_photonfrac_r.cpp:97-126: out[4] = {ray_count, return_count, escape_count, lost_count} (weighted sums);
 * the app's three fractions are out[1..3] / out[0].  _dev ADDS into d_out4 (4 doubles, zero first). */
int kr_reduce_return_f64(const kr_return_bins* b, const kr_ray_f64* rays, int64_t n, double out[4]);
int kr_reduce_return_dev_f64(const kr_return_bins* b, const void* d_rays, int64_t n, void* d_out4, void* stream);
/* range_phi(lo, hi) + kr_reduce_return_dev_f64 in one pass over the records (the returning-radiation driver's two passes after a trace) */
int kr_post_return_dev_f64(double lo, double hi, const kr_return_bins* b, void* d_rays, int64_t n, void* d_out4, void* stream);
/* kr_post_return_dev_f64 for `count` launches' rays at once: b, d_rays, n, d_out4 are HOST arrays of `count` entries (d_out4[i]: 4 doubles on the
 * device, ADDED into); the same rays[] and, up to the order of the additions, the same sums as `count` single calls, in ceil(count / 32) launches. */
int kr_post_return_batch_dev_f64(int32_t count, double lo, double hi, const kr_return_bins* b, void* const* d_rays, const int64_t* n, void* const* d_out4,
                                 void* stream);

/* ---- landing map of the returning radiation (kr_return_map above) ---------------------------------------------------------------------------
 * KR_EINVAL (message in kr_last_error) before anything touches a device: null pointers, n < 0, nr <= 0, count < 0.  Without a device: KR_ENODEVICE.
 * The _dev forms ADD into d_out (5 nr + 6 doubles on the device; zero it first) and neither wait for the device nor allocate;
 * kr_reduce_return_map_f64: host records, out = 5 nr + 6 host doubles (overwritten). */
int kr_reduce_return_map_f64(const kr_return_map* m, const kr_ray_f64* rays, int64_t n, double* out);
int kr_reduce_return_map_dev_f64(const kr_return_map* m, const void* d_rays, int64_t n, void* d_out, void* stream);
/* range_phi(lo, hi) + redshift(V, reverse, projradius, motion) + the classification on the wrapped phi + the map in ONE pass over the records (the
 * returning-radiation driver's passes after a trace, disc_source_photonfrac_r.cpp:93-126, with V = -1); rays[] ends up bit for bit as after
 * kr_range_phi_dev_f64 + kr_redshift_dev_f64 */
int kr_post_return_map_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_return_map* m, void* d_rays, int64_t n,
                               void* d_out, void* stream);
/* the same for `count` launches' rays at once: m, d_rays, n, d_out are HOST arrays of `count` entries (d_out[i]: 5 m[i].nr + 6 doubles on the device,
 * ADDED into; the nr may differ); the same rays[] and counts and, up to the order of the additions, the same sums as `count` single calls, in
 * ceil(count / 24) launches.  count == 0: KR_OK; an item with n[i] == 0 adds nothing. */
int kr_post_return_map_batch_dev_f64(int32_t count, double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_return_map* m,
                                     void* const* d_rays, const int64_t* n, void* const* d_out, void* stream);

/* ---- HEALPix point source and the fate map of its sky (kr_healpix_source, kr_healpix_map above) ------------------------------------------------
 * Every entry point checks its arguments before it touches a device (KR_EINVAL, message in kr_last_error): what kr_healpix_source refuses, null
 * pointers, first < 0, stride < 1, count < 0, a shard whose last pixel lies beyond the sphere (or beyond m->npix), a record count that is no
 * multiple of rays_per_pixel in the map passes.  Without a device: KR_ENODEVICE.  The _dev forms neither wait for the device nor allocate.
 * kr_healpix_count: rays_per_pixel * npix, npix in *npix when given; KR_EINVAL (negative) for a refused spec.
 * kr_healpix_vectors_dev_f64: the geometry alone -- for pixel first_pix + k stride, k < count, out[k] = four corners then the centre, 15 doubles.
 * kr_healpix_init_dev_f64: the records with emit = 0;  kr_healpix_init_emit_dev_f64: with their emitted energy, one pass;  `count` records.
 * kr_healpix_init_f64: the whole source into host records, n = kr_healpix_count(), staged through the device. */
int64_t kr_healpix_count(const kr_healpix_source* s, int64_t* npix);
int kr_healpix_vectors_dev_f64(int32_t order, int32_t unit_center, int64_t first_pix, int64_t stride, int64_t count, void* d_out, void* stream);
int kr_healpix_init_dev_f64(const kr_healpix_source* s, int64_t first, int64_t stride, void* d_rays, int64_t count, void* stream);
int kr_healpix_init_emit_dev_f64(const kr_healpix_source* s, int64_t first, int64_t stride, int reverse, void* d_rays, int64_t count, void* stream);
int kr_healpix_init_f64(const kr_healpix_source* s, kr_ray_f64* rays, int64_t n);
/* The fate pass over n records (n / rays_per_pixel pixels).  kr_post_: range_phi(lo, hi) + redshift(V, reverse, projradius, motion) on the centre
 * records, phi and g stored back as kr_range_phi_dev_f64 + kr_redshift_dev_f64 leave them (corner records are not touched), then the classes.
 * kr_reduce_: no wrap, no redshift, the records read as they are.  Both ADD the tallies into d_out (7 npix + 6 doubles; zero it first).
 * kr_reduce_healpix_map_f64: host records of the WHOLE sphere (first 0, stride 1), out = 7 npix + 6 host doubles (overwritten). */
int kr_post_healpix_map_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_healpix_map* m, void* d_rays,
                                int64_t n, int64_t first, int64_t stride, void* d_out, void* stream);
int kr_reduce_healpix_map_dev_f64(const kr_healpix_map* m, const void* d_rays, int64_t n, int64_t first, int64_t stride, void* d_out, void* stream);
int kr_reduce_healpix_map_f64(const kr_healpix_map* m, const kr_ray_f64* rays, int64_t n, double* out);

/* ---- point source with any four-velocity (kr_pointsource_vel_spec above has the rule and the refusals) -------------------------------------
 * Every entry point checks its arguments before it touches a device (KR_EINVAL, message in kr_last_error); without a device: KR_ENODEVICE.  The _dev
 * forms neither wait for the device nor allocate; the tetrad is solved on the host in each call and travels in the kernel's arguments.
 * kr_pointsource_vel_count: the ray count, the factors in *n_cosalpha / *n_beta when given; -1 for a null spec or a grid whose count is no int (it does
 *   not look at pos or u).
 * kr_pointsource_vel_tetrad: the sixteen doubles tetrad[leg][t, r, theta, phi] of a spec that passes every check (host only, no device needed).
 * kr_pointsource_vel_init_dev_f64: n = kr_pointsource_vel_count() records with emit = 0;  _init_emit_: with their emitted energy, one pass.
 * kr_pointsource_vel_init_f64: the same into host records, staged through the device. */
int64_t kr_pointsource_vel_count(const kr_pointsource_vel_spec* s, int32_t* n_cosalpha, int32_t* n_beta);
int kr_pointsource_vel_tetrad(const kr_pointsource_vel_spec* s, double* tetrad16);
int kr_pointsource_vel_init_dev_f64(const kr_pointsource_vel_spec* s, void* d_rays, int64_t n, void* stream);
int kr_pointsource_vel_init_emit_dev_f64(const kr_pointsource_vel_spec* s, void* d_rays, int64_t n, void* stream);
int kr_pointsource_vel_init_f64(const kr_pointsource_vel_spec* s, kr_ray_f64* rays, int64_t n);

/* ---- where a source's rays end, by emission angle (kr_angdist_spec above has the rule) ------------------------------------------------------
 * kr_angdist_nangle: Nangle of a spec, or -1 when it is refused.
 * kr_post_: range_phi(lo, hi) + redshift(V, reverse, projradius, motion) on every record, phi and g stored back as kr_range_phi_dev_f64 +
 * kr_redshift_dev_f64 leave them, then the reduction, in one pass.  kr_reduce_: no wrap, no redshift, the records read as they are.  Both ADD into d_out
 * (14 Nangle + 8 doubles on the device; zero it first).  n == 0 is KR_OK and adds nothing.  kr_reduce_angdist_f64: host records, out = 14 Nangle + 8
 * host doubles (overwritten). */
int kr_angdist_nangle(const kr_angdist_spec* sp);
int kr_post_angdist_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_angdist_spec* sp, void* d_rays,
                            int64_t n, void* d_out, void* stream);
int kr_reduce_angdist_dev_f64(const kr_angdist_spec* sp, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_angdist_f64(const kr_angdist_spec* sp, const kr_ray_f64* rays, int64_t n, double* out);

/* ---- the source-to-observer link: the direct continuum by observer inclination (kr_observer_spec above has the rule) ---------------------------
 * kr_post_: range_phi(lo, hi) + redshift(V, reverse, projradius, motion) on every record, phi and g stored back as kr_range_phi_dev_f64 +
 * kr_redshift_dev_f64 leave them, then the reduction, in one pass.  kr_reduce_: the records read as they are and never written.  Both ADD into d_out
 * (nmu (4 + nt) + 10 doubles on the device; zero it first).  n == 0 is KR_OK and adds nothing.  kr_reduce_observer_f64: host records, out =
 * nmu (4 + nt) + 10 host doubles (overwritten). */
int kr_post_observer_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_observer_spec* sp, void* d_rays,
                             int64_t n, void* d_out, void* stream);
int kr_reduce_observer_dev_f64(const kr_observer_spec* sp, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_observer_f64(const kr_observer_spec* sp, const kr_ray_f64* rays, int64_t n, double* out);

/* ---- the (r, phi) illumination map of the disc (kr_illum_bins above has the rule) ---------------------------------------------------------------
 * kr_post_: range_phi(lo, hi) + redshift(V, reverse, projradius, motion) on every record, stored back, then the map, in one pass: rays[] ends up
 * byte for byte as kr_post_emissivity_dev_f64 leaves it.  kr_reduce_: the records read as they are and never written.  Both ADD into d_out
 * (5 nr nphi + 2 doubles on the device; zero it first).  n == 0 is KR_OK and adds nothing.  kr_reduce_illum_f64: host records, out = 5 nr nphi + 2
 * host doubles (overwritten). */
int kr_post_illum_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_illum_bins* m, void* d_rays, int64_t n,
                          void* d_out, void* stream);
int kr_reduce_illum_dev_f64(const kr_illum_bins* m, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_illum_f64(const kr_illum_bins* m, const kr_ray_f64* rays, int64_t n, double* out);
/* the line and the response of an image plane's disc records driven by an (r, phi) table (kr_illum_table above has the rule): each is its flat twin with
 * the table as one more argument and the twin's output layout -- kr_post_line_illum: kr_post_line_limb_dev_f64 (2 nt ne + 3 doubles); kr_reduce_line_illum:
 * kr_reduce_line_dev_f64 / kr_reduce_line_f64 (2 nt ne + 2); kr_post_response_illum / kr_reduce_response_illum: kr_post_response_dev_f64 /
 * kr_reduce_response_dev_f64 / kr_reduce_response_f64 (nt ne + 4).  The device forms ADD into their buffer; the host forms overwrite out.  n == 0 is KR_OK. */
int kr_post_line_illum_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law,
                               const kr_illum_table* t, void* d_rays, int64_t n, void* d_line, void* stream);
int kr_reduce_line_illum_dev_f64(const kr_line_bins* b, const kr_illum_table* t, const void* d_rays, int64_t n, void* d_line, void* stream);
int kr_reduce_line_illum_f64(const kr_line_bins* b, const kr_illum_table* t, const kr_ray_f64* rays, int64_t n, double* out);
int kr_post_response_illum_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_response_model* r,
                                   const kr_limb_law* law, const kr_illum_table* t, void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_response_illum_dev_f64(const kr_response_model* r, const kr_illum_table* t, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_response_illum_f64(const kr_response_model* r, const kr_illum_table* t, const kr_ray_f64* rays, int64_t n, double* out);

/* ---- emission-line profile / transfer function (kr_line_bins above) --------------------------------------------------------------------
 * Every entry point validates the bins first, before it touches a device: KR_EINVAL (message in kr_last_error) when ne < 1 or nt < 1, de <= 0,
 * de <= 1 with log_e, e_min <= 0 with log_e, nt > 1 with dt <= 0, table_time without table_emis, table_nr < 1 with a table, a non-finite bin
 * parameter, or ne nt > 2^24.  The _dev forms ADD into d_line (2 nt ne + 2 doubles on the device; zero it first), so shards and batches of
 * rays can be summed.  kr_reduce_line_f64: host records, out = 2 nt ne + 2 host doubles (overwritten). */
int kr_reduce_line_f64(const kr_line_bins* b, const kr_ray_f64* rays, int64_t n, double* out);
int kr_reduce_line_dev_f64(const kr_line_bins* b, const void* d_rays, int64_t n, void* d_line, void* stream);
/* redshift(V, reverse, projradius, motion) + range_phi(lo, hi) + the line bins in one pass (the sibling of kr_post_image_dev_f64);
 * rays[] ends up exactly as after the separate calls */
int kr_post_line_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_line_bins* b, void* d_rays, int64_t n,
                         void* d_line, void* stream);
/* the notebook's per-pixel form over d_planes (7 img_nx img_ny + 1 doubles, the layout of kr_reduce_image_dev_f64) */
int kr_line_from_image_dev_f64(const kr_line_bins* b, const kr_image_bins* ib, const void* d_planes, void* d_line, void* stream);

/* ---- photon angles in the disc frame (kr_limb_law / kr_mu_bins above have the rule) ---------------------------------------------------------
 * Every entry point validates its arguments before it touches a device: KR_EINVAL (message in kr_last_error) for a null pointer, n < 0, a limb law
 * other than 0, 1, 2, nmu < 1, nr < 1, motion != 0 (only the orbiting observer has this frame) and whatever the line bins refuse.  n == 0 is KR_OK
 * and adds nothing.
 * kr_angles_dev_f64 reads the records and never writes them: d_angles[2 i] = mu, d_angles[2 i + 1] = chi (2 n doubles); NaN in both for a record with
 * steps <= 0; a bad-angle record gets its values as computed -- consumers filter.  kr_angles_f64: host records, host angles. */
int kr_angles_dev_f64(double spin, double V, int reverse, int projradius, int motion, const void* d_rays, int64_t n, void* d_angles, void* stream);
int kr_angles_f64(double spin, double V, int reverse, int projradius, int motion, const kr_ray_f64* rays, int64_t n, double* angles);
/* kr_post_line_dev_f64 with w *= limb(mu), mu from the metric and momentum evaluation that gives g: rays[] ends up exactly as after
 * kr_post_line_dev_f64.  ADDS into d_line, 2 nt ne + 3 doubles: the layout of kr_post_line_dev_f64, then bad_angle.  A bad-angle ray that passes the
 * filter counts in on_disc and bad_angle; with law != 0 it is not binned, with law 0 every ray is binned as kr_post_line_dev_f64 bins it. */
int kr_post_line_limb_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law,
                              void* d_rays, int64_t n, void* d_line, void* stream);
/* kr_post_emissivity_dev_f64 with the histogram split by incidence angle.  d_hist (5 nr + 1 doubles) receives exactly what kr_post_emissivity_dev_f64
 * puts there, bad-angle rays included, and rays[] ends up the same.  ADDS into d_mu, (2 nmu + 1) nr + 3 doubles:
 *   [count2 (nr x nmu: [ir nmu + im]) | flux2 (nr x nmu; each ray adds 1 / (num_primary_rays g)) | sum_mu (nr) | disc_count | binned | bad_angle]
 * A bad-angle ray that was binned radially moves only bad_angle: sum(count2) == binned - bad_angle, and each row of count2 sums to the radial count
 * minus that bin's bad-angle rays. */
int kr_post_emissivity_mu_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_emis_bins* b, const kr_mu_bins* mb,
                                  void* d_rays, int64_t n, void* d_hist, void* d_mu, void* stream);

/* ---- polarisation of disc emission on an image plane (kr_pol_law above has the rule) ------------------------------------------------------------
 * Every entry point validates its arguments before it touches a device: KR_EINVAL (message in kr_last_error) for a null pointer, n < 0, reverse != 1
 * (the rule is stated for image-plane records), motion != 0, a non-finite inc_deg, a bad limb law, a bad pol law, an image without pixels and whatever
 * the line bins refuse.  n == 0 is KR_OK and adds nothing.
 * kr_polarisation_dev_f64 reads the records and never writes them: d_out[4 i .. 4 i + 3] = {kappa1, kappa2, c2, s2} (4 n doubles); four NaNs for a
 * record with steps <= 0; a bad-pol record gets its values as computed -- consumers filter.  kr_polarisation_f64: host records, host output. */
int kr_polarisation_dev_f64(double spin, double V, int reverse, int projradius, int motion, double inc_deg, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_polarisation_f64(double spin, double V, int reverse, int projradius, int motion, double inc_deg, const kr_ray_f64* rays, int64_t n, double* out);
/* range_phi + redshift + the Stokes planes in one pass: rays[] ends up exactly as after kr_post_image_dev_f64, and the filter and the pixel rule are
 * its own (flip_image included; Q and U always refer to the plane's own x and y axes).  ADDS into d_stokes, 4 img_nx img_ny + 2 doubles:
 *   [nrays | I | Q | U] (each [ix img_ny + iy]) + disc_count, bad_pol
 * A ray that reaches a pixel and is not bad-pol adds 1, w, w delta c2, w delta s2 with w = powerlaw3(r) limb(mu) / g^3 (limb law 0: the FLUX plane's
 * term) and delta = the degree law at mu; a bad-pol ray that reaches a pixel moves only disc_count and bad_pol. */
int kr_post_image_stokes_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, double inc_deg, const kr_image_bins* b,
                                 const kr_limb_law* limb, const kr_pol_law* pol, void* d_rays, int64_t n, void* d_stokes, void* stream);
/* The energy-resolved form: the items of kr_post_line_limb_dev_f64 (E, w, tau, the bins, the table emissivity), each adding 1, w, w delta c2, w delta s2.
 * ADDS into d_out, 4 nt ne + 3 doubles: [count | I | Q | U] (nt x ne each) + on_disc, binned, bad_pol.  Bad-pol rays are never binned, whatever the limb
 * law.  rays[] ends up exactly as after kr_post_line_dev_f64. */
int kr_post_line_stokes_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, double inc_deg, const kr_line_bins* b,
                                const kr_limb_law* limb, const kr_pol_law* pol, void* d_rays, int64_t n, void* d_out, void* stream);

/* ---- continuum spectrum of the disc (kr_spectrum_model above has the rule) --------------------------------------------------------------------
 * Every entry point validates its arguments before it touches a device: KR_EINVAL (message in kr_last_error) for a null pointer, n < 0, whatever the
 * model's comment refuses, a limb law other than 0, 1, 2, and motion != 0 with a limb law other than 0 (only the orbiting observer has the frame of
 * mu).  n == 0 is KR_OK and adds nothing.  None of the _dev forms waits for the device or allocates, beyond the table cache's first copy of a table.
 * kr_post_spectrum_dev_f64: redshift(V, reverse, projradius, motion) + range_phi(lo, hi) + the spectrum in one pass; rays[] ends up exactly as after
 * kr_post_line_dev_f64.  ADDS into d_out (ne + 4 doubles; zero it first).
 * kr_reduce_spectrum_dev_f64: records that already carry their redshift; reads the records and never writes them; isotropic (law 0, no mu).
 * kr_reduce_spectrum_f64: host records, out = ne + 4 host doubles (overwritten). */
int kr_post_spectrum_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_spectrum_model* m,
                             const kr_limb_law* law, void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_spectrum_dev_f64(const kr_spectrum_model* m, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_spectrum_f64(const kr_spectrum_model* m, const kr_ray_f64* rays, int64_t n, double* out);
/* The Stokes spectra of the continuum (STOKES SPECTRA under kr_spectrum_model).  KR_EINVAL (message in kr_last_error) before a device is touched, and
 * nothing is written: V == KR_V_PLUNGE, whatever the model's comment refuses, reverse != 1, motion != 0, a non-finite inc_deg, a limb law other than 0, 1,
 * 2 or with a non-finite coeff, whatever kr_pol_law refuses, a null pointer, n < 0.  n == 0 is KR_OK and adds nothing.  None of the _dev forms waits for
 * the device or allocates, beyond the table cache's first copy of a table.
 * kr_post_spectrum_stokes_dev_f64: redshift(V, reverse, projradius, motion) + range_phi(lo, hi) + the Stokes spectra in one pass; rays[] ends up exactly
 * as after kr_post_spectrum_dev_f64, i.e. kr_post_line_dev_f64.  ADDS into d_out (3 ne + 4 doubles; zero it first).
 * kr_reduce_spectrum_stokes_dev_f64: records that already carry their redshift; reads the records and never writes them.
 * kr_reduce_spectrum_stokes_f64: host records, out = 3 ne + 4 host doubles (overwritten). */
int kr_post_spectrum_stokes_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, double inc_deg,
                                    const kr_spectrum_model* m, const kr_limb_law* law, const kr_pol_law* pol, void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_spectrum_stokes_dev_f64(double spin, double V, int reverse, int projradius, double inc_deg, const kr_spectrum_model* m,
                                      const kr_limb_law* law, const kr_pol_law* pol, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_spectrum_stokes_f64(double spin, double V, int reverse, int projradius, double inc_deg, const kr_spectrum_model* m,
                                  const kr_limb_law* law, const kr_pol_law* pol, const kr_ray_f64* rays, int64_t n, double* out);

/* ---- reverberation response of the disc (kr_response_model above has the rule) ---------------------------------------------------------------
 * Every entry point validates its arguments before it touches a device: KR_EINVAL (message in kr_last_error) for a null pointer, n < 0, whatever the
 * model's comment refuses, a limb law other than 0, 1, 2, and motion != 0 with a limb law other than 0.  n == 0 is KR_OK and adds nothing.  None of the
 * _dev forms waits for the device or allocates, beyond the table cache's first copy of a table.
 * kr_post_response_dev_f64: redshift(V, reverse, projradius, motion) + range_phi(lo, hi) + the response in one pass; rays[] ends up exactly as after
 * kr_post_line_dev_f64.  ADDS into d_out (nt ne + 4 doubles; zero it first).
 * kr_reduce_response_dev_f64: records that already carry their redshift; reads the records and never writes them; isotropic (law 0, no mu).
 * kr_reduce_response_f64: host records, out = nt ne + 4 host doubles (overwritten). */
int kr_post_response_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_response_model* r,
                             const kr_limb_law* law, void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_response_dev_f64(const kr_response_model* r, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_response_f64(const kr_response_model* r, const kr_ray_f64* rays, int64_t n, double* out);

/* ---- the line, the continuum, the response and the angles of rays that LANDED ON THE SURFACE of a disc (kr_disc_surface above has the rule) -------
 * Each entry point takes the surface and what its flat twin takes without V, projradius and motion: the observer is the Keplerian gas at rho.  Every
 * one validates its arguments before it touches a device: KR_EINVAL (message in kr_last_error, naming the parameter) for a null surface, whatever
 * KR_STOP_THICKDISC refuses of its stop_params, a null pointer, n < 0, and whatever the flat twin refuses of the bins, the model and the limb law.
 * n == 0 is KR_OK and adds nothing.
 * kr_angles_surface_dev_f64: d_angles[2 i] = mu, d_angles[2 i + 1] = chi to the surface normal for every record with steps > 0, whatever it landed on
 * (NaN in both otherwise); reads the records and never writes them.  kr_angles_surface_f64: host records, host angles.
 * kr_post_*_surface_dev_f64: range_phi(lo, hi) + redshift(V = -1, reverse, projradius = 1, motion = 0) + the pass; rays[] ends up exactly as after
 * kr_post_image_surface_dev_f64.  The layouts are the flat passes' word for word: the line 2 nt ne + 3 doubles (kr_post_line_limb_dev_f64's), the
 * spectrum ne + 4, the response nt ne + 4.  All ADD into their output.
 * kr_reduce_*_surface_dev_f64: records that carry their redshift and wrapped phi; read only; isotropic (the line's bad_angle word stays 0).  The _f64
 * forms take host records and overwrite host output. */
int kr_angles_surface_dev_f64(const kr_disc_surface* s, double spin, int reverse, const void* d_rays, int64_t n, void* d_angles, void* stream);
int kr_angles_surface_f64(const kr_disc_surface* s, double spin, int reverse, const kr_ray_f64* rays, int64_t n, double* angles);
int kr_post_line_surface_dev_f64(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law,
                                 void* d_rays, int64_t n, void* d_line, void* stream);
int kr_reduce_line_surface_dev_f64(const kr_disc_surface* s, const kr_line_bins* b, const void* d_rays, int64_t n, void* d_line, void* stream);
int kr_post_spectrum_surface_dev_f64(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_spectrum_model* m,
                                     const kr_limb_law* law, void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_spectrum_surface_dev_f64(const kr_disc_surface* s, const kr_spectrum_model* m, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_spectrum_surface_f64(const kr_disc_surface* s, const kr_spectrum_model* m, const kr_ray_f64* rays, int64_t n, double* out);
int kr_post_response_surface_dev_f64(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_response_model* r,
                                     const kr_limb_law* law, void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_response_surface_dev_f64(const kr_disc_surface* s, const kr_response_model* r, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_response_surface_f64(const kr_disc_surface* s, const kr_response_model* r, const kr_ray_f64* rays, int64_t n, double* out);

/* ---- orbiting hot spot on the disc (kr_hotspot above has the rule) ------------------------------------------------------------------------------
 * Every entry point validates its arguments before it touches a device: KR_EINVAL (message in kr_last_error) for a null pointer, n < 0, whatever the
 * spot's comment refuses, a limb law other than 0, 1, 2, and motion != 0 with a limb law other than 0.  n == 0 is KR_OK and adds nothing.  None of the
 * _dev forms waits for the device or allocates.
 * kr_post_hotspot_dev_f64: redshift(V, reverse, projradius, motion) + range_phi(lo, hi) + the spot in one pass; rays[] ends up exactly as after
 * kr_post_line_dev_f64.  ADDS into d_out (nt (3 + ne) + 4 doubles; zero it first).
 * kr_reduce_hotspot_dev_f64: records that already carry their redshift and wrapped phi; reads the records and never writes them; isotropic.
 * kr_reduce_hotspot_f64: host records, out = nt (3 + ne) + 4 host doubles (overwritten). */
int kr_post_hotspot_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_hotspot* h, const kr_limb_law* law,
                            void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_hotspot_dev_f64(const kr_hotspot* h, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_hotspot_f64(const kr_hotspot* h, const kr_ray_f64* rays, int64_t n, double* out);
/* The Stokes light curves of the spot (the Stokes rule under kr_hotspot).  KR_EINVAL (message in kr_last_error) before a device is touched, and nothing is
 * written: V == KR_V_PLUNGE, whatever the spot's comment refuses, reverse != 1, motion != 0, a non-finite inc_deg, a limb law other than 0, 1, 2 or with a
 * non-finite coeff, whatever kr_pol_law refuses, a null pointer, n < 0.  n == 0 is KR_OK and adds nothing.  None of the _dev forms waits for the device or
 * allocates.
 * kr_post_hotspot_stokes_dev_f64: redshift(V, reverse, projradius, motion) + range_phi(lo, hi) + the spot with its Stokes sums in one pass; rays[] ends up
 * exactly as after kr_post_line_dev_f64.  ADDS into d_out (nt (5 + ne) + 4 doubles; zero it first).
 * kr_reduce_hotspot_stokes_dev_f64: records that already carry their redshift and wrapped phi (every further spot on the same plane); reads the records
 * and never writes them.
 * kr_reduce_hotspot_stokes_f64: host records, out = nt (5 + ne) + 4 host doubles (overwritten). */
int kr_post_hotspot_stokes_dev_f64(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, double inc_deg, const kr_hotspot* h,
                                   const kr_limb_law* law, const kr_pol_law* pol, void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_hotspot_stokes_dev_f64(double spin, double V, int reverse, int projradius, double inc_deg, const kr_hotspot* h, const kr_limb_law* law,
                                     const kr_pol_law* pol, const void* d_rays, int64_t n, void* d_out, void* stream);
int kr_reduce_hotspot_stokes_f64(double spin, double V, int reverse, int projradius, double inc_deg, const kr_hotspot* h, const kr_limb_law* law,
                                 const kr_pol_law* pol, const kr_ray_f64* rays, int64_t n, double* out);

/* ---- critical-curve maps (kr_caustic_map above): caustic_discplane.cpp on the device -------------------------------------------------------
 * Every entry point validates its arguments before it touches a device: KR_EINVAL (message in kr_last_error) when nx or ny < 1, eps_x or eps_y
 * is <= 0 or non-finite, eps_frac <= 0 or >= 0.5 (the constructor), or n is smaller than 5 nx ny (bundles) / nx ny (grid).  None of them waits
 * for the device, allocates or frees.
 * kr_bundles_init_emit_dev_f64: the ImagePlaneBundles constructor (imageplane_bundles.h:150-199) + redshift_start(V, reverse, projradius) in one
 * pass (ImagePlaneBundles::redshift_start() is V = 0, reverse = 1): record s is member s % 5 (centre, east, west, north, south; satellites eps_frac of
 * a grid step away) of bundle s / 5, bundle b the grid point (b / ny, b % ny) of kr_imageplane_init_emit_dev_f64; the same per-ray arithmetic, except
 * that the point x = y = 0 takes beta = 0 (as the host mirror's constructor) instead of asin(0 / 0).  Records from 5 nx ny on get steps = -1. */
int kr_bundles_init_emit_dev_f64(const kr_imageplane* s, double eps_frac, double V, int reverse, int projradius, void* d_rays, int64_t n, void* stream);
/* redshift(dest, reverse) of every record (rays[].redshift exactly as after kr_redshift_dest_dev_f64; `spin` as stored by the Raytracer, i.e.
 * negated) + the nine planes and the six counts in one pass over the records (caustic_discplane.cpp:217-334; bundles = 0: :349-439, the Jacobian by a
 * second pass over the planes).  WRITES every word of d_maps (suppressed = 0). */
int kr_post_caustic_disc_dev_f64(double spin, int reverse, const kr_caustic_map* m, void* d_rays, int64_t n, void* d_maps, void* stream);
/* branch-boundary suppression (caustic_discplane.cpp:455-493): a pixel with SIGN_J != 0 whose 4-neighbourhood -- in the planes as they are when the
 * call is made -- holds more opposite than equal signs, and at least two opposite ones, gets DET_J = 1e30, SIGN_J = 0; their number -> suppressed */
int kr_caustic_suppress_dev_f64(const kr_caustic_map* m, void* d_maps, void* stream);
/* the gather and the Jacobian of caustic_sourceplane.cpp:180-232, :264-305 (kind = 0) and caustic_plane.cpp:207-299 / :315-392 (kind = 1) over traced
 * records (kr_source_map above): rays from kr_imageplane_init_dev_f64 (grid) or kr_bundles_init_emit_dev_f64 (bundles; its `emit` is not read), traced
 * with stop_kind = KR_STOP_THETA, theta_max = 0, r_max = r_lim, or to KR_STOP_FLATPLANE.  The records are only read; those from nx ny (grid) or 5 nx ny
 * (bundles) on are ignored.  WRITES every word of d_maps.  KR_EINVAL (message in kr_last_error) before anything touches a device when the map is
 * null, nx or ny < 1, eps_x or eps_y is <= 0 or non-finite, the kind is unknown, kind = 0 comes with bundles, a sine or cosine of kind = 1 is not
 * finite, or n is smaller than 5 nx ny (bundles) / nx ny (grid).  Does not wait for the device, allocate or free. */
int kr_post_caustic_source_dev_f64(const kr_source_map* m, const void* d_rays, int64_t n, void* d_maps, void* stream);

/* ---- diagnostics ------------------------------------------------------------------------------- */
/* out[i] = op(a[i], b[i]) evaluated ON THE DEVICE with the exact primitive the trace kernel uses (host pointers):
 * 0 a/b (compiler IEEE)  1 a/b (lean IEEE chain of the strict path)  2 sqrt(a) (compiler)  3 sqrt(a) (lean)
 * 4 sin(a)  5 cos(a) (compact polar-angle sincos)  6 a*rcp(b)  7 sqrt(a) (fast-math path)  8 sin  9 cos  10 pow(a,b) (device libm)
 * 11-18 further primitives of the two arithmetic paths (kr_post.hip::arith_probe_kernel)  19 a after 20 000 additions of b (kr_replay.hpp)
 * 20 1.2345678901234567 / ((a a) b), 21 b / (a a) through the assembled reciprocals of one derivative evaluation (kr_device.hpp::StageRecips)
 * 22 acos(a)  23 asin(a)  24 atan2(a, b)  25 tan(a): the correctly rounded routines of the device ImagePlane constructor (kr_crmath.hpp)
 * 26-28 work on PAIRS of elements (i even): out[i] is what a lane gets that takes a wave-uniform shortcut of the fast Euler / RK4 step when its guard lets
 * it, out[i + 1] what the code behind the guard gives for the same operands -- 26 the capped step: step = a[i], num = a[i + 1], m = b[i];  27, 28 the end of
 * a step at r = a[i], theta = a[i + 1] from theta_prev = b[i + 1] with theta_max = b[i], horizon 1.0625, r_max 1000: 27 the outcome as finished + 2 HORIZON +
 * 4 crossings + 8 (thetadot_sign flipped) + 16 (phi moved), 28 theta afterwards (kr_post.hip::probe_step_end)
 * 29 works on GROUPS of eight elements (i a multiple of 8; b is not read): one stage evaluation of the fast RK4 step at a[i .. i + 7] = r, theta0, d, k,
 * h, Q, spin, signs (bit 0: rdot_sign = -1, bit 1: thetadot_sign = -1) -- the stage angle is theta0 + d, its sine and cosine by angle addition from the base
 * point's pair: out[i .. i + 7] = tdot, rdot, thetadot, phidot, tdot and phidot as they were associated before P / (rho^2 Delta) was shared, the sine, the
 * cosine (kr_post.hip::probe_fast_stage) */
int kr_debug_arith_f64(int op, const double* a, const double* b, double* out, int64_t n);

/* ---- a long-lived host ray array (what Raytracer<T> holds as `rays`) ----------------------------- */
/* kr_host_attach keeps a device buffer for the array until kr_host_detach.  Host-pointer entry points called on an attached array
 * (or on a sub-range of it) allocate nothing and copy back only what their pass modifies: `emit` (redshift_start), `phi` (range_phi), `redshift` (redshift*), the four momenta (calculate_momentum),
 * the whole record (trace, the source constructors).  Semantics are unchanged: the host array is the input of every call and is
 * complete when the call returns.  ray_bytes = sizeof(kr_ray_f64) or sizeof(kr_ray_f32).  Detach before freeing the array. */
int kr_host_attach(void* rays, int64_t n, int32_t ray_bytes);
int kr_host_detach(void* rays);

/* ---- device memory helpers for callers without a HIP runtime of their own --------------------- */
int kr_malloc(void** d_ptr, int64_t bytes);
int kr_free(void* d_ptr);
/* page-locked host memory: kr_memcpy_* to / from it run at full PCIe rate without a staging copy or first-touch faults */
int kr_host_alloc(void** h_ptr, int64_t bytes);
int kr_host_free(void* h_ptr);
int kr_memcpy_h2d(void* d_dst, const void* h_src, int64_t bytes);
int kr_memcpy_d2h(void* h_dst, const void* d_src, int64_t bytes);
int kr_memset(void* d_ptr, int value, int64_t bytes);
int kr_synchronize(void* stream);
/* streams for such callers (hipStreamCreateWithFlags(hipStreamNonBlocking) / hipStreamDestroy); the handle is what the *_dev
 * entry points take as `stream` */
int kr_stream_create(void** stream);
int kr_stream_destroy(void* stream);                /* also releases the internal side stream split traces on `stream` used */
/* Hardware queues.  Traces are meant to overlap (a split trace uses two streams, a multi-launch driver keeps many in flight) and the
 * HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues per device -- 4 by default: 18 concurrent RK45 sweep points take
 * 1.65 s on 4 queues, 0.76 s on 16 (profiles/r02_hw_queues.txt).  The variable is read when the runtime initialises, and it is
 * process-global: the library does NOT touch it when it is loaded.  An application that owns its process calls kr_configure_process() FIRST (before
 * any other HIP user -- this library, PyTorch, RCCL -- starts the runtime); it sets GPU_MAX_HW_QUEUES=16 unless the user chose a value.
 * Returns 1 if it set (or found) the variable before THIS LIBRARY touched the runtime, 0 if this library already had: it cannot see whether another
 * HIP user in the process (PyTorch, RCCL) started the runtime earlier -- then the setting comes too late and 1 is returned all the same.  The Python
 * package sets the default in raytrace_cpu_amd/__init__.py, i.e. at import, before `import torch` can start the runtime; bench.py, the kr_* apps
 * and the class mirror call this function first thing. */
int kr_configure_process(void);
/* Waits for the devices the library has used, then releases every pooled trace workspace, internal stream and device table (the PointSource angle
 * tables and the line emissivity tables).  Refused with KR_EINVAL (nothing released) while a ticket of kr_trace_async_* / kr_trace_batch_async_f64
 * is outstanding: wait for or release the tickets first.
 * Optional, and never done implicitly: at process exit the HIP runtime may already be gone when this library is unloaded. */
int kr_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif /* KR_TRACE_H_ */
