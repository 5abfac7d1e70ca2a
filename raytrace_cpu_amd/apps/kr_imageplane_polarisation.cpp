// apps/kr_imageplane_polarisation.cpp -- the polarised image of an accretion disc: kr_imageplane_disc_image's pipeline (image-plane rays generated,
// traced to the disc and reduced in HBM) with the Stokes planes of kr_post_image_stokes_dev_f64 as its last pass (include/kr_trace.h, kr_pol_law: the
// emitted polarisation lies in the disc plane, perpendicular to the projected photon direction in the frame of the orbiting gas, and is carried to the
// image plane by the Walker-Penrose constant).  The reference has no such program.
//
// Reads the keys of kr_imageplane_disc_image (--parfile, --outfile | outfile, dist, --incl | incl, plane_phi0, --spin | spin, r_disc, x0, xmax, Nx, y0,
// ymax, Ny, img_Nx, img_Ny, q1, rb1, q2, rb2, q3, precision, flip_image, integrator, rk45_tol; --integrator, --arithmetic | KRTRACE_ARITHMETIC, --device,
// --timing), plus
//   pol_law = 1, pol_coeff = 0.1171   the degree law: 0 constant, 1 coeff (1 - mu) / (1 + 3.582 mu) (Chandrasekhar's scattering atmosphere)
//   limb = 0, limb_coeff = 2.06       the limb law of the intensity (kr_limb_law)
//   spec_outfile, en0 = 1, enmax = 10, Nen = 90, line_energy = 6.4
//                                     with spec_outfile: the energy-resolved table `E I Q U PDEG EVPA` of a line at line_energy from the same
//                                     records (kr_post_line_stokes_dev_f64), Nen linear bins of [en0, enmax), E the bin's middle
// Writes a 6-HDU FITS file (an empty primary + NRAYS, I, Q, U, PDEG, EVPA): NRAYS, I, Q, U are the sums over the rays of a pixel, PDEG =
// sqrt(Q^2 + U^2) / I (NaN where I = 0), EVPA = atan2(U, Q) / 2 in degrees, from the image's x axis towards its y axis.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/kerr.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "../host/include/text_output.h"
#include "app_common.h"
#include "disc_image_fits.h"

using krapp::AxisInfo;

namespace {
double pdeg_of(double I, double Q, double U) { return I == 0 ? NAN : sqrt(Q * Q + U * U) / I; }
double evpa_deg_of(double Q, double U) { return 0.5 * atan2(U, Q) * 180 / M_PI; }
}  // namespace

int main(int argc, char** argv)
try {
    (void) kr_configure_process();       // first HIP user of this process: hardware queues for overlapping launches (include/kr_trace.h)
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/imageplane_disc_image.par");
    ParameterFile par(par_name);
    auto num = [&](const string& key, double dflt) { return args.key_exists("--" + key) ? args.get_parameter<double>("--" + key) : par.get_parameter<double>(key, dflt); };
    auto str = [&](const string& key, const string& dflt) { return args.key_exists("--" + key) ? args.get_parameter<string>("--" + key) : par.get_parameter<string>(key, dflt); };

    const string out_name = args.key_exists("--outfile") ? args.get_parameter<string>("--outfile") : par.get_parameter<string>("outfile");
    const double dist = par.get_parameter<double>("dist");
    const double incl = args.key_exists("--incl") ? args.get_parameter<double>("--incl") : par.get_parameter<double>("incl");
    const double plane_phi0 = par.get_parameter<double>("plane_phi0", 0);
    const double spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
    const double r_disc = par.get_parameter<double>("r_disc");
    AxisInfo ax;
    ax.x0 = par.get_parameter<double>("x0", -1 * r_disc);
    ax.xmax = par.get_parameter<double>("xmax", r_disc);
    const int Nx = par.get_parameter<int>("Nx");
    ax.y0 = par.get_parameter<double>("y0", ax.x0);
    ax.ymax = par.get_parameter<double>("ymax", ax.xmax);
    const int Ny = par.get_parameter<int>("Ny", Nx);
    ax.img_nx = par.get_parameter<int>("img_Nx", Nx);
    ax.img_ny = par.get_parameter<int>("img_Ny", ax.img_nx);
    const double q1 = par.get_parameter<double>("q1", 3), rb1 = par.get_parameter<double>("rb1", 4), q2 = par.get_parameter<double>("q2", 3),
                 rb2 = par.get_parameter<double>("rb2", 10), q3 = par.get_parameter<double>("q3", 3);
    const double precision = par.get_parameter<double>("precision", 100);
    const bool flip_image = par.get_parameter<bool>("flip_image", true);
    const string integ = args.key_exists("--integrator") ? args.get_parameter<string>("--integrator") : par.get_parameter<string>("integrator", "rk45");
    const double rk45_tol = par.get_parameter<double>("rk45_tol", 1e-8);
    const string arith = args.key_exists("--arithmetic") ? args.get_parameter<string>("--arithmetic") : krapp::arithmetic_from_env();
    const bool timing = args.key_exists("--timing");

    kr_pol_law pol;
    memset(&pol, 0, sizeof pol);
    pol.law = (int32_t) num("pol_law", 1);
    pol.coeff = num("pol_coeff", 0.1171);
    kr_limb_law limb;
    memset(&limb, 0, sizeof limb);
    limb.law = (int32_t) num("limb", 0);
    limb.coeff = num("limb_coeff", 2.06);
    const string spec_name = str("spec_outfile", "");
    const double en0 = num("en0", 1), enmax = num("enmax", 10), line_energy = num("line_energy", 6.4);
    const int Nen = (int) num("Nen", 90);

    ax.dx = (ax.xmax - ax.x0) / Nx;
    ax.dy = (ax.ymax - ax.y0) / Ny;
    const double r_isco = kerr_isco<double>(spin, +1);
    cout << "ISCO at " << r_isco << endl;

    kr_imageplane plane;
    memset(&plane, 0, sizeof plane);
    plane.dist = dist;
    plane.inc_deg = incl;
    plane.x0 = ax.x0; plane.xmax = ax.xmax; plane.dx = ax.dx;
    plane.y0 = ax.y0; plane.ymax = ax.ymax; plane.dy = ax.dy;
    plane.spin = spin;
    plane.phi0 = plane_phi0;
    plane.precision = precision;

    kr_image_bins bins;
    memset(&bins, 0, sizeof bins);
    bins.x0 = ax.x0; bins.y0 = ax.y0;
    bins.img_dx = (ax.xmax - ax.x0) / ax.img_nx;
    bins.img_dy = (ax.ymax - ax.y0) / ax.img_ny;
    bins.r_isco = r_isco; bins.r_disc = r_disc;
    bins.q1 = q1; bins.rb1 = rb1; bins.q2 = q2; bins.rb2 = rb2; bins.q3 = q3;
    bins.img_nx = ax.img_nx; bins.img_ny = ax.img_ny;
    bins.flip_image = flip_image ? 1 : 0;

    kr_line_bins lb;
    memset(&lb, 0, sizeof lb);
    lb.line_energy = line_energy;
    lb.e_min = en0; lb.de = (enmax - en0) / Nen; lb.ne = Nen;
    lb.nt = 1;
    lb.r_isco = r_isco; lb.r_disc = r_disc;
    lb.q1 = q1; lb.rb1 = rb1; lb.q2 = q2; lb.rb2 = rb2; lb.q3 = q3;
    lb.g_index = 3;

    kr_params p;
    kr_params_default(&p, -spin);            // the image plane traces backwards in time: spin enters negated (imageplane.cpp:12)
    p.precision = precision;
    p.integrator = krapp::integrator_code(integ, KR_RK45);
    if (p.integrator == KR_RK45) p.rk45_tol = rk45_tol;
    p.theta_max = M_PI_2;
    p.r_max = 1.1 * dist;
    p.stop_kind = KR_STOP_THETA;
    p.flags = krapp::arithmetic_flags(arith, p.integrator);

    // ---- device pipeline: init_emit -> trace -> redshift + range_phi + Stokes planes (-> Stokes line from the same records) ----------------
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch clock;
    const int64_t n = kr_imageplane_count(&plane, nullptr, nullptr);
    if (n <= 0) throw runtime_error("empty ray grid");
    if (ax.img_nx <= 0 || ax.img_ny <= 0) throw runtime_error("image size must be positive");
    const int64_t npix = (int64_t) ax.img_nx * ax.img_ny;
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    krapp::DeviceBuffer stokes((4 * npix + 2) * (int64_t) sizeof(double));
    stokes.zero();
    krapp::check(kr_imageplane_init_emit_dev_f64(&plane, 0, 1, 0.0, 1, 0, rays.get(), n, nullptr), "imageplane_init + redshift_start");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_init = clock.lap_ms();
    kr_stats st;
    krapp::check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &st), "trace");
    const double ms_trace = clock.lap_ms();
    krapp::check(kr_post_image_stokes_dev_f64(-spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, incl, &bins, &limb, &pol, rays.get(), n, stokes.get(), nullptr),
                 "redshift + range_phi + Stokes planes");
    krapp::PinnedDoubles h(6 * npix + 2);      // [NRAYS | I | Q | U | disc_count, bad_pol] read back, then PDEG and EVPA behind them
    krapp::check(kr_memcpy_d2h(h.data(), stokes.get(), (4 * npix + 2) * (int64_t) sizeof(double)), "d2h");
    vector<double> line;
    if (!spec_name.empty()) {
        // the records keep their geodesic and `emit`: the second pass writes the redshift and the wrapped phi that the first one left
        const int64_t words = 4 * (int64_t) Nen + 3;
        krapp::DeviceBuffer d_line(words * (int64_t) sizeof(double));
        d_line.zero();
        krapp::check(kr_post_line_stokes_dev_f64(-spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, incl, &lb, &limb, &pol, rays.get(), n, d_line.get(), nullptr),
                     "redshift + range_phi + Stokes line");
        line.resize((size_t) words);
        krapp::check(kr_memcpy_d2h(line.data(), d_line.get(), words * (int64_t) sizeof(double)), "d2h");
    }
    const double ms_post = clock.lap_ms();

    double* hp = h.data();
    const long disc_count = static_cast<long>(hp[4 * npix]), bad_pol = static_cast<long>(hp[4 * npix + 1]);
    cout << disc_count << " rays hit the disc, " << bad_pol << " of them without a polarisation angle (bad-pol)" << endl;
    double* pdeg = hp + 4 * npix;              // over the two tallies, which have been read
    double* evpa = hp + 5 * npix;
    krapp::parallel_for(npix, [=](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; ++i) {
            const double I = hp[npix + i], Q = hp[2 * npix + i], U = hp[3 * npix + i];
            pdeg[i] = pdeg_of(I, Q, U);
            evpa[i] = evpa_deg_of(Q, U);
        }
    });

    // ---- FITS: the primary header of the disc image, one extension per plane with its axis keywords ----------------------------------------
    {
        vector<vector<double*>> rows(6, vector<double*>(static_cast<size_t>(ax.img_nx)));
        for (int k = 0; k < 6; ++k)
            for (int ix = 0; ix < ax.img_nx; ++ix) rows[k][ix] = hp + k * npix + static_cast<int64_t>(ix) * ax.img_ny;
        FITSOutput<double> fits(out_name);
        fits.create_primary();
        fits.write_comment("Polarised raytraced images of accretion disc");
        fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "kr_imageplane_polarisation");
        fits.write_keyword("raytrace_source", "Raytrace source configuration", "imageplane");
        fits.write_keyword("DIST", "Distance to image plane", dist);
        fits.write_keyword("INCL", "Inclination of line of sight", incl);
        fits.write_keyword("SPIN", "Black hole spin", spin);
        fits.write_keyword("ISCO", "Innermost stable circular orbit", r_isco);
        fits.write_keyword("RDISC", "Maximum radius of disc", r_disc);
        fits.write_keyword("Q1", "Emissivity profile inner power law index", q1);
        fits.write_keyword("RB1", "Emissivity profile inner break radius", rb1);
        fits.write_keyword("Q2", "Emissivity profile middle power law index", q2);
        fits.write_keyword("RB2", "Emissivity profile outer break radius", rb2);
        fits.write_keyword("Q3", "Emissivity profile outer power law index", q3);
        fits.write_keyword("POLLAW", "Polarisation degree law", (int) pol.law);
        fits.write_keyword("POLCOEF", "Polarisation degree coefficient", pol.coeff);
        fits.write_keyword("LIMB", "Limb law of the intensity", (int) limb.law);
        fits.write_keyword("LIMBCOEF", "Limb law coefficient", limb.coeff);
        fits.write_keyword("NRAYS", "Number of rays", Nx * Ny);
        fits.write_keyword("DISCRAYS", "Rays hitting disc", disc_count);
        fits.write_keyword("BADPOL", "Disc rays without a polarisation angle", bad_pol);
        krapp::write_plane(fits, rows[0].data(), "NRAYS", "Rays per pixel", "COUNT", "RAYS", ax);
        krapp::write_plane(fits, rows[1].data(), "I", "Stokes I, summed over the rays of a pixel", "FLUX", "PH*EN^2/DT", ax);
        krapp::write_plane(fits, rows[2].data(), "Q", "Stokes Q on the image axes, summed over the rays of a pixel", "FLUX", "PH*EN^2/DT", ax);
        krapp::write_plane(fits, rows[3].data(), "U", "Stokes U on the image axes, summed over the rays of a pixel", "FLUX", "PH*EN^2/DT", ax);
        krapp::write_plane(fits, rows[4].data(), "PDEG", "Polarisation degree sqrt(Q^2 + U^2) / I", "FRACTION", "NONE", ax);
        krapp::write_plane(fits, rows[5].data(), "EVPA", "Polarisation angle from the image X axis towards Y", "ANGLE", "DEG", ax);
        fits.close();
    }

    if (!spec_name.empty()) {
        cout << static_cast<long>(line[4 * (size_t) Nen]) << " rays on the disc, " << static_cast<long>(line[4 * (size_t) Nen + 1]) << " binned" << endl;
        TextOutput outfile(spec_name);
        for (int i = 0; i < Nen; ++i) {
            const double I = line[(size_t) Nen + i], Q = line[2 * (size_t) Nen + i], U = line[3 * (size_t) Nen + i];
            outfile << en0 + (i + 0.5) * lb.de << I << Q << U << pdeg_of(I, Q, U) << evpa_deg_of(Q, U) << endl;
        }
    }
    const double ms_out = clock.lap_ms();

    if (timing)
        cout << "timing: rays " << st.rays_traced << " steps " << st.steps_total << " | init+redshift_start " << ms_init << " ms | trace " << ms_trace
             << " ms (kernel " << st.kernel_ms << ") | redshift+range_phi+Stokes+readback " << ms_post << " ms | output files " << ms_out << " ms" << endl;
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
