// apps/kr_imageplane_polarisation.cpp -- the polarised image of an accretion disc: kr_imageplane_disc_image's pipeline (image-plane rays generated,
// traced to the disc and reduced in HBM) with the Stokes planes of kr_post_image_stokes_dev_f64 as its last pass (include/kr_trace.h, kr_pol_law: the
// emitted polarisation lies in the disc plane, perpendicular to the projected photon direction in the frame of the orbiting gas, and is carried to the
// image plane by the Walker-Penrose constant).  The reference has no such program.
//
// Reads the parameter file of kr_imageplane_disc_image and the plane and disc keys of imageplane_app.h (--parfile, outfile, dist, incl, plane_phi0, spin,
// r_disc, x0, xmax, Nx, y0, ymax, Ny, img_Nx, img_Ny, q1, rb1, q2, rb2, q3, precision, flip_image, integrator, rk45_tol; --arithmetic | KRTRACE_ARITHMETIC,
// --device, --timing), plus
//   pol_law = 1, pol_coeff = 0.1171   the degree law: 0 constant, 1 coeff (1 - mu) / (1 + 3.582 mu) (Chandrasekhar's scattering atmosphere)
//   limb = 0, limb_coeff = 2.06       the limb law of the intensity (kr_limb_law)
//   spec_outfile, en0 = 1, enmax = 10, Nen = 90, line_energy = 6.4
//                                     with spec_outfile: the energy-resolved table `E I Q U PDEG EVPA` of a line at line_energy from the same
//                                     records (kr_post_line_stokes_dev_f64), Nen linear bins of [en0, enmax), E the bin's middle
// Every key may also be given as --key=value, which takes precedence over the file (before imageplane_app.h the plane and disc keys other than
// outfile, incl, spin and integrator could not; such arguments were ignored), and `device` may stand in the file.
// Writes a 6-HDU FITS file (an empty primary + NRAYS, I, Q, U, PDEG, EVPA): NRAYS, I, Q, U are the sums over the rays of a pixel, PDEG =
// sqrt(Q^2 + U^2) / I (NaN where I = 0), EVPA = atan2(U, Q) / 2 in degrees, from the image's x axis towards its y axis.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/text_output.h"
#include "imageplane_app.h"

namespace {
double pdeg_of(double I, double Q, double U) { return I == 0 ? NAN : sqrt(Q * Q + U * U) / I; }
double evpa_deg_of(double Q, double U) { return 0.5 * atan2(U, Q) * 180 / M_PI; }
}  // namespace

static void program(const krapp::Options& opt)
{
    const krapp::DiscPlaneSetup s(opt);
    const kr_pol_law pol = krapp::pol_law_of(opt);
    kr_limb_law limb;
    memset(&limb, 0, sizeof limb);
    limb.law = (int32_t) opt.num("limb", 0);
    limb.coeff = opt.num("limb_coeff", 2.06);
    const string spec_name = opt.str("spec_outfile", "");
    const double en0 = opt.num("en0", 1), enmax = opt.num("enmax", 10), line_energy = opt.num("line_energy", 6.4);
    const int Nen = (int) opt.num("Nen", 90);
    s.print_isco();

    const kr_imageplane plane = s.plane();
    const kr_image_bins bins = s.image_bins();
    kr_line_bins lb;
    memset(&lb, 0, sizeof lb);
    lb.line_energy = line_energy;
    lb.e_min = en0; lb.de = (enmax - en0) / Nen; lb.ne = Nen;
    lb.nt = 1;
    s.fill_disc(lb);
    lb.g_index = 3;
    const kr_params p = s.params(KR_RK45);

    // ---- device pipeline: init_emit -> trace -> redshift + range_phi + Stokes planes (-> Stokes line from the same records) ----------------
    krapp::DiscPlaneRun run(s, plane);
    if (s.ax.img_nx <= 0 || s.ax.img_ny <= 0) throw runtime_error("image size must be positive");
    const int64_t npix = (int64_t) s.ax.img_nx * s.ax.img_ny;
    run.trace(plane, p, 4 * npix + 2);
    void *rays = run.rays->get(), *stokes = run.acc->get();
    krapp::check(kr_post_image_stokes_dev_f64(-s.spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, s.incl, &bins, &limb, &pol, rays, run.n, stokes, nullptr),
                 "redshift + range_phi + Stokes planes");
    krapp::PinnedDoubles h(6 * npix + 2);      // [NRAYS | I | Q | U | disc_count, bad_pol] read back, then PDEG and EVPA behind them
    krapp::check(kr_memcpy_d2h(h.data(), stokes, (4 * npix + 2) * (int64_t) sizeof(double)), "d2h");
    vector<double> line;
    if (!spec_name.empty()) {
        // the records keep their geodesic and `emit`: the second pass writes the redshift and the wrapped phi that the first one left
        const int64_t words = 4 * (int64_t) Nen + 3;
        krapp::DeviceBuffer d_line(words * (int64_t) sizeof(double));
        d_line.zero();
        krapp::check(kr_post_line_stokes_dev_f64(-s.spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, s.incl, &lb, &limb, &pol, rays, run.n, d_line.get(), nullptr),
                     "redshift + range_phi + Stokes line");
        line.resize((size_t) words);
        krapp::check(kr_memcpy_d2h(line.data(), d_line.get(), words * (int64_t) sizeof(double)), "d2h");
    }
    const double ms_post = run.clock.lap_ms();

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
        vector<vector<double*>> rows(6, vector<double*>(static_cast<size_t>(s.ax.img_nx)));
        for (int k = 0; k < 6; ++k)
            for (int ix = 0; ix < s.ax.img_nx; ++ix) rows[k][ix] = hp + k * npix + static_cast<int64_t>(ix) * s.ax.img_ny;
        FITSOutput<double> fits(s.out_name);
        fits.create_primary();
        fits.write_comment("Polarised raytraced images of accretion disc");
        fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "kr_imageplane_polarisation");
        fits.write_keyword("raytrace_source", "Raytrace source configuration", "imageplane");
        fits.write_keyword("DIST", "Distance to image plane", s.dist);
        fits.write_keyword("INCL", "Inclination of line of sight", s.incl);
        fits.write_keyword("SPIN", "Black hole spin", s.spin);
        fits.write_keyword("ISCO", "Innermost stable circular orbit", s.r_isco);
        fits.write_keyword("RDISC", "Maximum radius of disc", s.r_disc);
        fits.write_keyword("Q1", "Emissivity profile inner power law index", s.q1);
        fits.write_keyword("RB1", "Emissivity profile inner break radius", s.rb1);
        fits.write_keyword("Q2", "Emissivity profile middle power law index", s.q2);
        fits.write_keyword("RB2", "Emissivity profile outer break radius", s.rb2);
        fits.write_keyword("Q3", "Emissivity profile outer power law index", s.q3);
        fits.write_keyword("POLLAW", "Polarisation degree law", (int) pol.law);
        fits.write_keyword("POLCOEF", "Polarisation degree coefficient", pol.coeff);
        fits.write_keyword("LIMB", "Limb law of the intensity", (int) limb.law);
        fits.write_keyword("LIMBCOEF", "Limb law coefficient", limb.coeff);
        fits.write_keyword("NRAYS", "Number of rays", s.Nx * s.Ny);
        fits.write_keyword("DISCRAYS", "Rays hitting disc", disc_count);
        fits.write_keyword("BADPOL", "Disc rays without a polarisation angle", bad_pol);
        krapp::write_plane(fits, rows[0].data(), "NRAYS", "Rays per pixel", "COUNT", "RAYS", s.ax);
        krapp::write_plane(fits, rows[1].data(), "I", "Stokes I, summed over the rays of a pixel", "FLUX", "PH*EN^2/DT", s.ax);
        krapp::write_plane(fits, rows[2].data(), "Q", "Stokes Q on the image axes, summed over the rays of a pixel", "FLUX", "PH*EN^2/DT", s.ax);
        krapp::write_plane(fits, rows[3].data(), "U", "Stokes U on the image axes, summed over the rays of a pixel", "FLUX", "PH*EN^2/DT", s.ax);
        krapp::write_plane(fits, rows[4].data(), "PDEG", "Polarisation degree sqrt(Q^2 + U^2) / I", "FRACTION", "NONE", s.ax);
        krapp::write_plane(fits, rows[5].data(), "EVPA", "Polarisation angle from the image X axis towards Y", "ANGLE", "DEG", s.ax);
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
    const double ms_out = run.clock.lap_ms();

    if (s.timing) run.print_timing() << "redshift+range_phi+Stokes+readback " << ms_post << " ms | output files " << ms_out << " ms" << endl;
}

int main(int argc, char** argv) { return krapp::run_program(argc, argv, "../par/imageplane_disc_image.par", program); }
