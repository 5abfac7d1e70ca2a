// kr_disc_pass.hpp -- what the passes over the rays that end on the disc share (kr_line.hip, kr_spectrum.hip, kr_hotspot.hip): the disc filter, the per-ray
// front end of the fused and reduce forms, the tile compactor of the two-phase kernels, the two bin coordinates, and on the host the slot dispatch, the
// isotropic law and the energy-axis validation.  The device helpers are forced-inline functions, as in kr_pass.hpp.  Three places repeat a helper written
// out, each with a comment that names it, because the call changes their code: image_accumulate (kr_post.hip) and stokes_pixel (kr_polarisation.hip) the
// filter, hotspot_kernel the front end and the compactor, which it measures 1 ... 3 % slower through (profiles/disc_pass_shared_ab.txt).
#pragma once

#include <cmath>
#include <type_traits>

#include "kr_pass.hpp"

namespace kr {

// ---- device side --------------------------------------------------------------------------------------------------------------------------
// the disc filter of imageplane_disc_image.cpp:127-128 without the pixel-range test: the ray was traced, ended in the equatorial plane between
// r_isco and r_disc, and has a redshift (a NaN in r or g fails)
KR_DEV bool disc_filter(double r_isco, double r_disc, int steps, double r, double theta, double g)
{
    if (!(steps > 0)) return false;
    const double z = r * kr_cos(theta);
    return z < 1E-2 && r >= r_isco && r < r_disc && g > 0;
}

// ---- the emission angle on a disc with a SURFACE |z| = H(rho) (include/kr_trace.h, kr_disc_surface; a compile-time parameter of the disc passes like
//      DiscFlow (kr_post_device.hpp), so that every flat instance is the code it was).  DiscSurface<false> carries nothing; DiscSurface<true> what
//      H'(rho) needs.  The frame is frame_value_coef's (kr_post_device.hpp) with V = -1 and projradius = 1 (the Keplerian observer at
//      rho = r sin(theta)): frame_value expression for expression -- E keeps redshift_value's bits -- handing on the sine and cosine of theta and the
//      two metric coefficients that put the gradient of sg z - H(rho) on the legs e3, e2.  The gas moves in phi only and the surface depends on
//      neither t nor phi: the normal is orthogonal to the gas four-velocity and the boost leaves e2, e3 alone, so this is the proper normal in the
//      gas frame. ----
template <bool SURFACE> struct DiscSurface {};
template <> struct DiscSurface<true> { double r_in, slope, scale; };

// mu = |P_n| / E, the cosine to the surface normal, and P_s, the momentum along the surface away from the axis (chi = atan2(P_phi, P_s)); nn is the
// length of the unnormalised normal.  One IEEE operation per line of the rule in include/kr_trace.h, in its association.
struct SurfaceAngle { double mu, P_s, nn; };

KR_DEV SurfaceAngle surface_angle(const DiscSurface<true>& sf, const Frame& f, const FrameCoef& mc, double r)
{
    const double sn = mc.sn, cs = mc.cs;
    const double rho = r * sn, z = r * cs;
    const double sg = z < 0 ? -1.0 : 1.0;
    const double Hp = sf.slope + (sf.scale * 0.5 * kr_sqrt(sf.r_in / rho)) / rho;
    const double f_r = sg * cs - Hp * sn;
    const double f_th = -1 * (sg * (r * sn)) - Hp * (r * cs);
    const double n_r = kr_sqrt(mc.delta / mc.rhosq) * f_r;
    const double n_th = f_th / kr_sqrt(mc.rhosq);
    SurfaceAngle s;
    s.nn = kr_sqrt(n_r * n_r + n_th * n_th);
    const double P_n = (n_r * f.P_r + n_th * f.P_th) / s.nn;
    s.mu = kr_abs(P_n) / f.E;
    s.P_s = sg * (n_r * f.P_th - n_th * f.P_r) / s.nn;
    return s;
}

KR_DEV bool surface_bad_angle(const Frame& f, const SurfaceAngle& s) { return frame_bad_angle(f, s.mu) || !__builtin_isfinite(s.nn) || s.nn == 0; }

// what H'(rho) needs of a kr_disc_surface that surface_validate has passed (host side)
inline DiscSurface<true> surface_dev(const kr_disc_surface* s)
{
    DiscSurface<true> sf;
    sf.r_in = s->r_in; sf.slope = s->slope; sf.scale = s->scale;
    return sf;
}

// the filter of a record that LANDED ON A SURFACE (image_surface_kernel, kr_surface.hip): traced, stopped by the destination, with a redshift, and its
// cylindrical radius rho = r sin(theta) between r_isco and r_disc (a NaN in rho or g fails)
KR_DEV bool disc_filter_surface(double r_isco, double r_disc, int steps, int status, double rho, double g)
{
    return steps > 0 && (status & KR_STATUS_DEST) != 0 && g > 0 && rho >= r_isco && rho < r_disc;
}

// what the front end hands to a pass's own *_item: the end point, the redshift, the wrapped phi and the limb weight (1 where no law applies)
struct DiscRay { double r, theta, g, phi, limb; };

// One record up to the pass's own item.  FUSED: redshift + range_phi (rays[] ends as after post_line_kernel: g and mu come from ONE metric and
// momentum evaluation, frame_value, whose E is redshift_value's recv to the bit), then the filter, mu and the limb law; motion != 0 takes
// redshift_value and no angle (law 0 only: the validators refuse the rest).  Otherwise the record carries its redshift and wrapped phi and is only
// read.  A ray that passes the filter counts in on_disc; one whose emission angle is bad counts in bad_angle too and, under law 0, is used like
// every other ray; under the other laws -- whose weight it would poison -- it is dropped.  Returns false for a dropped ray.
// (One drop flag and one assignment of the outputs at the end, not early returns: those cost the fused kernels two VGPRs.)
// PLUNGE: the disc flow of KR_V_PLUNGE (DiscFlow, kr_post_device.hpp) in the fused form with motion 0; DiscFlow<false> is today's code.
// SURFACE: the record landed on the surface of kr_disc_surface (DiscSurface, kr_post_device.hpp).  The observer is V = -1 at rho with motion 0 whatever
// V, projradius and motion say, the filter is disc_filter_surface, mu is the cosine to the surface normal, and out->r is rho: every radius that a pass's
// item takes is the cylindrical one.  DiscSurface<false> is today's code.
template <bool FUSED, bool PLUNGE, bool SURFACE = false, class Ray>
KR_DEV bool disc_ray(Ray* ray, double r_isco, double r_disc, double spin, double V, int reverse, int projradius, int motion, double lo, double hi,
                     const kr_limb_law& law, DiscRay* out, unsigned long long& on_disc, unsigned long long& bad_angle, const DiscFlow<PLUNGE>& fl,
                     const DiscSurface<SURFACE>& sf = DiscSurface<SURFACE>{})
{
    static_assert(!(SURFACE && PLUNGE), "the surface passes keep the Keplerian observer at rho");
    double r, theta, g, phi, limb = 1;
    const int steps = ray->steps;
    bool drop = false;
    if constexpr (SURFACE) {
        double rho;
        [[maybe_unused]] Frame f;
        [[maybe_unused]] FrameCoef mc;
        if constexpr (FUSED) {
            const kr_ray_f64 v = geodesic_of(ray);
            theta = v.theta;
            f = frame_value_coef(v, spin, -1.0, reverse, 1, &mc);
            g = frame_redshift(f, v.emit, reverse);
            ray->redshift = g;
            phi = wrap_phi(ray, steps, lo, hi);
            r = v.r;
            rho = r * mc.sn;
        } else {
            r = ray->r; theta = ray->theta; g = ray->redshift; phi = ray->phi;
            rho = r * kr_sin(theta);
        }
        if (disc_filter_surface(r_isco, r_disc, steps, ray->status, rho, g)) {
            on_disc++;
            if constexpr (FUSED) {
                const SurfaceAngle s = surface_angle(sf, f, mc, r);
                if (surface_bad_angle(f, s)) {
                    bad_angle++;
                    drop = law.law != 0;
                }
                limb = limb_weight(law.law, law.coeff, s.mu);
            }
        } else {
            drop = true;
        }
        r = rho;
    } else if constexpr (FUSED) {
        const kr_ray_f64 v = geodesic_of(ray);
        r = v.r; theta = v.theta;
        if (motion == 0) {
            const Frame f = frame_value<PLUNGE>(v, spin, V, reverse, projradius, fl);
            g = frame_redshift(f, v.emit, reverse);
            ray->redshift = g;
            phi = wrap_phi(ray, steps, lo, hi);
            if (disc_filter(r_isco, r_disc, steps, r, theta, g)) {
                on_disc++;
                const double mu = frame_mu(f);
                if (frame_bad_angle(f, mu)) {
                    bad_angle++;
                    drop = law.law != 0;
                }
                limb = limb_weight(law.law, law.coeff, mu);
            } else {
                drop = true;
            }
        } else {
            g = redshift_value(v, spin, V, reverse, projradius, motion);
            ray->redshift = g;
            phi = wrap_phi(ray, steps, lo, hi);
            if (disc_filter(r_isco, r_disc, steps, r, theta, g)) on_disc++;
            else drop = true;
        }
    } else {
        r = ray->r; theta = ray->theta; g = ray->redshift; phi = ray->phi;
        if (disc_filter(r_isco, r_disc, steps, r, theta, g)) on_disc++;
        else drop = true;
    }
    out->r = r; out->theta = theta; out->g = g; out->phi = phi; out->limb = limb;
    return !drop;
}

// Compaction of one tile of kBlock lanes: the live lanes get consecutive places at = 0 ... items - 1 (a ballot per wave, the waves' counts through
// wave_count[kBlock / 64] in LDS and ONE barrier, a prefix over the waves).  The caller stores its item at [at] (at < items <= kBlock), issues the
// second barrier and reads the items.  No third barrier closes the tile: a wave that runs ahead into the next tile writes wave_count, which every
// wave has read before the second barrier, and the item arrays only after the next tile's first barrier, which no wave passes while another still
// reads items.  So between the second barrier and the next tile_compact the caller must touch neither wave_count nor the item arrays except to read
// the items; every lane of the workgroup calls this, in every tile.
KR_DEV void tile_compact(bool live, int* wave_count, int* at, int* items)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(live);
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int place = __popcll(mask & ((1ull << lane) - 1)), total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; w++) {
        const int cnt = wave_count[w];
        if (w < wave) place += cnt;
        total += cnt;
    }
    *at = place;
    *items = total;
}

// the emissivity app's index into a radial table (emissivity.cpp:106): truncation, so (-1, nr) is the range that lands in [0, nr); false when r falls
// outside the table (a NaN too).  (One division of the chosen operands, here and below: the form the compiler gives the expression written out.)
KR_DEV bool radial_table_index(int logbin, double r_min, double dr, double log_dr, int nr, double r, int* ir)
{
    const double fi = (logbin ? kr_log(r / r_min) : r - r_min) / (logbin ? log_dr : dr);
    if (!(fi > -1 && fi < nr)) return false;
    *ir = (int) fi;
    return true;
}

// ---- the (r, phi) illumination table of the line and the response (include/kr_trace.h, kr_illum_table): a compile-time parameter of their kernels like
//      DiscFlow and DiscSurface, so that every instance without it is the code it was.  IllumTab<false> carries nothing; IllumTab<true> the table's
//      grid, the device copies of its planes (global memory: nr nphi doubles each) and the two values taken once on the host. ----
template <bool ILLUM> struct IllumTab {};
template <> struct IllumTab<true> {
    double r_min, dr, log_dr, phi_shift, dphi;       // log_dr: log(dr) with logbin; dphi = 2 M_PI / nphi
    const double* emis;                              // [nr nphi] on the device
    const double* time;                              // [nr nphi] on the device, or null
    int nr, nphi, logbin;
};

// emis and tt of a disc record at (r, phi): the radial index of radial_table_index, the azimuthal cell of kr_illum_bins (kr_illum.hip).  false: the
// record has no cell (no ir, a q_ph that is not >= 0) or its cell holds a non-finite emis or tt -- it is not used
KR_DEV bool illum_table_entry(const IllumTab<true>& T, double r, double phi, double* emis, double* tt)
{
    int ir, ip = 0;
    if (!radial_table_index(T.logbin, T.r_min, T.dr, T.log_dr, T.nr, r, &ir)) return false;
    if (T.nphi != 1) {
        const double p = phi + T.phi_shift;
        const double phi_w = p - (2 * kPi) * floor((p + kPi) / (2 * kPi));
        const double q_ph = (phi_w + kPi) / T.dphi;
        if (!(q_ph >= 0)) return false;
        ip = q_ph < T.nphi ? (int) q_ph : T.nphi - 1;
    }
    const int c = ir * T.nphi + ip;
    if (!(c >= 0 && c < T.nr * T.nphi)) return false;
    const double e = T.emis[c], t = T.time ? T.time[c] : 0;
    if (!__builtin_isfinite(e) || !__builtin_isfinite(t)) return false;
    *emis = e; *tt = t;
    return true;
}

// the energy E in units of bins from e_min; the bin is (int) of it where 0 <= it < ne (the caller's test: a NaN fails)
KR_DEV double energy_bin_coord(int log_e, double e_min, double de, double log_de, double E)
{
    return (log_e ? kr_log(E / e_min) : E - e_min) / (log_e ? log_de : de);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
constexpr int kMaxSlots = 16;            // a lane of a two-phase kernel owns at most this many outputs: ne, nt <= kMaxSlots kBlock = 4096

// f(std::integral_constant<int, K>) for the compiled slot count K = 1, 2, 4, 8 or kMaxSlots that holds `slots`
template <typename F>
void for_slots(int slots, F f)
{
    if (slots <= 1) f(std::integral_constant<int, 1>{});
    else if (slots <= 2) f(std::integral_constant<int, 2>{});
    else if (slots <= 4) f(std::integral_constant<int, 4>{});
    else if (slots <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, kMaxSlots>{});
}

// the law of the reduce forms, whose records carry no emission angle
inline kr_limb_law isotropic_limb()
{
    kr_limb_law iso;
    iso.coeff = 0; iso.law = 0; iso.pad = 0;
    return iso;
}

// a kr_illum_table that illum_table_validate (kr_pass.hpp) has passed: its planes on the device through the table store (kr_illum.hip), pinned in
// `pins`: keep it until the kernel that reads them has been enqueued
int illum_table_dev(const kr_illum_table* t, TablePins& pins, IllumTab<true>* T);

// the energy axis of kr_line_bins, kr_spectrum_model and kr_hotspot; bad(why) sets the error and returns its code
template <typename Bad>
int energy_axis_validate(Bad bad, double de, int log_e, double e_min)
{
    if (!(de > 0)) return bad("de must be positive");
    if (log_e && !(de > 1)) return bad("log_e: de (the ratio between edges) must be > 1");
    if (log_e && !(e_min > 0)) return bad("log_e: e_min must be positive");
    return KR_OK;
}

}  // namespace kr
