// apps/kr_offaxis_reverb.cpp -- the reverberation response of a disc lit by a source that is NOT on the axis, resident on the MI355X from start to
// finish: the source's rays are traced to the disc and binned into the (r, phi) illumination map (kr_illum_bins: kr_post_illum_dev_f64), the map becomes
// the table of emissivity and source -> disc delay per cell (kr_illum_table), and the image plane's disc rays read it by their own (r, phi) in the
// energy-time response of a tabulated rest-frame spectrum (kr_post_response_illum_dev_f64).  Only the map's 5 Nr Nphi + 2 words and the response's
// Nt x Nen + 4 words come back (include/kr_trace.h has both rules).
//
// Reads the plane and disc keys of imageplane_app.h and the limb keys of kr_line_profile (--parfile, outfile, dist, incl, plane_phi0, spin, r_disc, x0,
// xmax, Nx, y0, ymax, Ny, limb, limb_coeff, precision, integrator, rk45_tol; --arithmetic, --device, --timing), and
//   source_r, source_theta, source_phi = 0, source_V = 0   the point source (kr_pointsource: its position and orbital velocity d phi / d t)
//   dcosalpha, dbeta                  the source's ray grid over cos(alpha) in [-0.995, 0.995] and beta in [-pi, pi]
//   source_rmax = 1000                the source's rays are traced to the disc plane within this radius
//   Nr = 50, Nphi = 32, logbin = 1    the disc grid of the map and the table: Nr rings from the ISCO to r_disc, Nphi cells of 2 pi / Nphi from phi = -pi
//   gamma = 2                         the photon index of the map's emissivity plane, emis += g^-gamma
//   phase = 0                         the orbital phase of the source: the map is made ONCE for the source at source_phi and read as the table of the
//                                     source at source_phi + phase, table.phi_shift = -phase (the metric is axisymmetric)
//   e_min = 0.1, e_max = 10, Nen = 100, log_e = 1, spec_file, Nzones, spec_bins = 512, t0 = dist, dt = 1, Nt = 100   as kr_reverb_response reads them
// Every key may also be given as --key=value, which takes precedence over the file.
// Table: emis = emis_sum / (area / Nphi) with area = integrate_disc_area(r_i, r_i+1, spin, circular orbits, dphi = 2 pi) of host/include/disc.h, the
// proper area of the ring; time = sum_time / count, NaN in a cell no ray reached -- the disc records of such a cell are not used.
// Output: a FITS file (host/include/fits_output.h).  The primary HDU (EXTNAME RESPONSE) holds the response, Nen pixels along axis 1 and Nt along axis 2,
// with the tallies of both passes (ON_DISC, USED, BADANGLE, OUTSIDE; SRC_DISC, SRC_BIN) and the parameters as header keys; the HDUs ILLUM_EMIS,
// ILLUM_TIME and ILLUM_COUNT hold the table and the map's ray counts, Nphi pixels along axis 1 and Nr along axis 2, and ILLUM_AREA the Nr ring areas.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/disc.h"
#include "../host/include/fits_output.h"
#include "imageplane_app.h"
#include "rest_spectrum.h"

static void program(const krapp::Options& opt)
{
    const krapp::DiscPlaneSetup s(opt, false);
    kr_limb_law limb;
    memset(&limb, 0, sizeof limb);
    limb.law = (int32_t) opt.num("limb", 0);
    limb.coeff = opt.num("limb_coeff", 2.06);

    const double source_r = opt.req("source_r"), source_theta = opt.req("source_theta"), source_phi = opt.num("source_phi", 0), source_V = opt.num("source_V", 0);
    const double dcosalpha = opt.req("dcosalpha"), dbeta = opt.req("dbeta"), source_rmax = opt.num("source_rmax", 1000);
    const int nr = opt.integer("Nr", 50), nphi = opt.integer("Nphi", 32);
    const bool logbin = opt.num("logbin", 1) != 0;
    const double gamma = opt.num("gamma", 2), phase = opt.num("phase", 0);
    if (nr < 1 || nphi < 1 || (int64_t) nr * nphi > ((int64_t) 1 << 20)) throw invalid_argument("Nr, Nphi: at least one ring and one cell, at most 2^20 cells");

    const double e_min = opt.num("e_min", 0.1), e_max = opt.num("e_max", 10);
    const int ne = (int) opt.num("Nen", 100);
    const bool log_e = opt.num("log_e", 1) != 0;
    if (ne < 1) throw invalid_argument("Nen: at least one energy");
    const double de = log_e ? exp(log(e_max / e_min) / ne) : (e_max - e_min) / ne;
    const double t0 = opt.num("t0", s.dist), dt = opt.num("dt", 1);
    const int nt = (int) opt.num("Nt", 100);
    if (nt < 1) throw invalid_argument("Nt: at least one time row");
    s.print_isco();

    // ---- the source and the map's bins ---------------------------------------------------------------------------------------------------------
    kr_pointsource ps;
    memset(&ps, 0, sizeof ps);
    ps.pos[0] = 0; ps.pos[1] = source_r; ps.pos[2] = source_theta; ps.pos[3] = source_phi;
    ps.V = source_V; ps.spin = s.spin; ps.tol = 100; ps.E = 1;
    ps.dcosalpha = dcosalpha; ps.dbeta = dbeta; ps.cosalpha0 = -0.995; ps.cosalphamax = 0.995; ps.beta0 = -1 * M_PI; ps.betamax = M_PI;
    const int64_t n_src = kr_pointsource_count(&ps, nullptr, nullptr);
    if (n_src <= 0) throw runtime_error("the source's grid gives no rays");
    kr_illum_bins map;
    memset(&map, 0, sizeof map);
    map.rad.r_min = s.r_isco;
    map.rad.dr = logbin ? exp(log(s.r_disc / s.r_isco) / nr) : (s.r_disc - s.r_isco) / nr;
    map.rad.r_isco = s.r_isco; map.rad.gamma = gamma; map.rad.spin = s.spin; map.rad.num_primary_rays = (double) n_src;
    map.rad.nr = nr; map.rad.logbin = logbin ? 1 : 0;
    map.phi_shift = 0; map.nphi = nphi;
    kr_params p_src;
    kr_params_default(&p_src, s.spin);
    p_src.integrator = krapp::integrator_code(s.integ, KR_RK4);
    if (p_src.integrator == KR_RK45) p_src.rk45_tol = s.rk45_tol;
    p_src.theta_max = M_PI_2;
    p_src.r_max = source_rmax;
    p_src.stop_kind = KR_STOP_THETA;
    p_src.flags = krapp::arithmetic_flags(s.arith, p_src.integrator);

    const kr_imageplane plane = s.plane();
    kr_response_model rm;
    memset(&rm, 0, sizeof rm);
    kr_spectrum_model& sm = rm.spec;
    sm.e_min = e_min; sm.de = de; sm.ne = ne; sm.log_e = log_e ? 1 : 0;
    s.fill_disc(sm);
    sm.f_col = 1;
    rm.t0 = t0; rm.dt = dt; rm.nt = nt;
    const krapp::RestSpectrum rest = krapp::read_rest_spectrum(opt, "kr_offaxis_reverb needs spec_file");
    rest.fill(sm);
    rest.print();
    const kr_params p = s.params(KR_RK45);

    // ---- device pipeline, source side: init_emit -> trace -> range_phi + redshift + map -----------------------------------------------------------
    krapp::DiscPlaneRun run(s, plane);                       // (kr_set_device; the image plane's ray buffer)
    const int64_t ncell = (int64_t) nr * nphi, map_words = 5 * ncell + 2;
    vector<double> m((size_t) map_words);
    {
        krapp::DeviceBuffer src_rays(n_src * (int64_t) sizeof(kr_ray_f64)), src_out(map_words * (int64_t) sizeof(double));
        src_out.zero();
        krapp::check(kr_pointsource_init_emit_dev_f64(&ps, 0, 1, source_V, 0, 0, src_rays.get(), n_src, nullptr), "point source + redshift_start");
        kr_stats st;
        memset(&st, 0, sizeof st);
        krapp::check(kr_trace_dev_f64(&p_src, src_rays.get(), n_src, nullptr, &st), "trace of the source's rays");
        krapp::check(kr_post_illum_dev_f64(s.spin, -1.0, 0, 0, 0, -1 * M_PI, M_PI, &map, src_rays.get(), n_src, src_out.get(), nullptr), "range_phi + redshift + illumination map");
        krapp::check(kr_memcpy_d2h(m.data(), src_out.get(), map_words * (int64_t) sizeof(double)), "d2h");
    }
    const long src_disc = static_cast<long>(m[(size_t) (5 * ncell)]), src_binned = static_cast<long>(m[(size_t) (5 * ncell + 1)]);
    cout << n_src << " source rays, " << src_disc << " on the disc, " << src_binned << " in the " << nr << " x " << nphi << " cells of the map" << endl;

    // ---- the table: emis = emis_sum / (area / Nphi), time = sum_time / count (NaN where no ray landed) ---------------------------------------------
    vector<double> area((size_t) nr), emis((size_t) ncell), delay((size_t) ncell), count(m.begin(), m.begin() + ncell);
    for (int i = 0; i < nr; ++i) {
        const double lo = logbin ? map.rad.r_min * pow(map.rad.dr, i) : map.rad.r_min + i * map.rad.dr;
        const double hi = logbin ? map.rad.r_min * pow(map.rad.dr, i + 1) : map.rad.r_min + (i + 1) * map.rad.dr;
        area[(size_t) i] = integrate_disc_area<double>(lo, hi, s.spin, true, 50, 2 * M_PI);
        for (int k = 0; k < nphi; ++k) {
            const size_t c = (size_t) i * nphi + k;
            emis[c] = m[(size_t) (2 * ncell) + c] / (area[(size_t) i] / nphi);
            delay[c] = count[c] > 0 ? m[(size_t) (4 * ncell) + c] / count[c] : (double) NAN;
        }
    }
    kr_illum_table table;
    memset(&table, 0, sizeof table);
    table.r_min = map.rad.r_min; table.dr = map.rad.dr; table.phi_shift = -1 * phase;
    table.emis = emis.data(); table.time = delay.data();
    table.nr = nr; table.nphi = nphi; table.logbin = map.rad.logbin;

    // ---- observer side: init_emit -> trace -> redshift + range_phi + response read from the table ---------------------------------------------------
    const int64_t cells = (int64_t) nt * ne, words = cells + 4;
    run.trace(plane, p, words);
    krapp::check(kr_post_response_illum_dev_f64(-s.spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, &rm, &limb, &table, run.rays->get(), run.n, run.acc->get(), nullptr),
                 "redshift + range_phi + response from the (r, phi) table");
    vector<double> h((size_t) words);
    krapp::check(kr_memcpy_d2h(h.data(), run.acc->get(), words * (int64_t) sizeof(double)), "d2h");
    const double ms_post = run.clock.lap_ms();
    const long on_disc = static_cast<long>(h[(size_t) cells]), used = static_cast<long>(h[(size_t) cells + 1]), bad_angle = static_cast<long>(h[(size_t) cells + 2]),
               outside = static_cast<long>(h[(size_t) cells + 3]);
    cout << on_disc << " rays on the disc, " << used << " used, " << bad_angle << " without an emission angle (bad-angle), " << outside << " outside the time window" << endl;
    {
        FITSOutput<double> fits(s.out_name);
        fits.write_image_array(h.data(), ne, nt);
        fits.set_ext_name("RESPONSE");
        fits.write_comment("Energy-time response of a disc lit by an off-axis source: axis 1 energy, axis 2 time");
        fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "kr_offaxis_reverb");
        fits.write_keyword("DIST", "Distance to image plane", s.dist);
        fits.write_keyword("INCL", "Inclination of line of sight", s.incl);
        fits.write_keyword("SPIN", "Black hole spin", s.spin);
        fits.write_keyword("ISCO", "Innermost stable circular orbit", s.r_isco);
        fits.write_keyword("RDISC", "Maximum radius of disc", s.r_disc);
        fits.write_keyword("SRC_R", "Source radius", source_r);
        fits.write_keyword("SRC_TH", "Source polar angle", source_theta);
        fits.write_keyword("SRC_PHI", "Source azimuth of the traced map", source_phi);
        fits.write_keyword("SRC_V", "Source angular velocity", source_V);
        fits.write_keyword("PHASE", "Orbital phase added to the source azimuth", phase);
        fits.write_keyword("PHISHIFT", "phi_shift of the table", table.phi_shift);
        fits.write_keyword("SRC_RAYS", "Number of source rays", static_cast<long>(n_src));
        fits.write_keyword("SRC_DISC", "Source rays hitting disc", src_disc);
        fits.write_keyword("SRC_BIN", "Source rays in a cell of the map", src_binned);
        fits.write_keyword("NR", "Rings of the map", nr);
        fits.write_keyword("NPHI", "Azimuthal cells of the map", nphi);
        fits.write_keyword("NRAYS", "Number of image-plane rays", static_cast<long>(run.n));
        fits.write_keyword("ON_DISC", "Rays hitting disc", on_disc);
        fits.write_keyword("USED", "Rays with an emissivity and a delay", used);
        fits.write_keyword("BADANGLE", "Rays on the disc without an emission angle", bad_angle);
        fits.write_keyword("OUTSIDE", "Used rays outside the time window", outside);
        fits.write_keyword("T0", "Start of the first time row (GM/c^3)", t0);
        fits.write_keyword("DT", "Width of a time row (GM/c^3)", dt);
        fits.write_keyword("NT", "Number of time rows", nt);
        fits.write_keyword("E_MIN", "Lower edge of the first energy bin", e_min);
        fits.write_keyword("DE", log_e ? "Ratio between energy bin edges" : "Width of an energy bin", de);
        fits.write_keyword("NEN", "Number of energies", ne);
        fits.write_keyword("LOG_E", "Logarithmic energy bins", log_e);
        fits.write_image_array(emis.data(), nphi, nr);
        fits.set_ext_name("ILLUM_EMIS");
        fits.write_comment("Emissivity per cell of the disc: axis 1 azimuth from -pi, axis 2 radius");
        fits.write_image_array(delay.data(), nphi, nr);
        fits.set_ext_name("ILLUM_TIME");
        fits.write_comment("Mean source -> disc delay per cell; NaN where no ray landed");
        fits.write_image_array(count.data(), nphi, nr);
        fits.set_ext_name("ILLUM_COUNT");
        fits.write_comment("Source rays per cell");
        fits.write_image_array(area.data(), nr, 1);
        fits.set_ext_name("ILLUM_AREA");
        fits.write_comment("Proper area of each ring");
        fits.close();
    }
    const double ms_out = run.clock.lap_ms();
    if (s.timing) run.print_timing() << "redshift+range_phi+response+readback " << ms_post << " ms | FITS file " << ms_out << " ms" << endl;
}

int main(int argc, char** argv) { return krapp::run_program(argc, argv, "../par/offaxis_reverb.par", program); }
