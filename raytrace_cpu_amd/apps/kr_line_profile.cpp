// apps/kr_line_profile.cpp -- the relativistically broadened emission line (and, with a time axis, the reverberation transfer function) of
// the disc seen on an image plane, resident on the MI355X from start to finish.  The reference builds the line outside its C++: it writes the
// image FITS file with imageplane_disc_image and sums ENSHIFT / RADIUS pixels into energy bins in python/line_from_image.ipynb.  Here the rays
// are generated, traced, redshifted and binned in HBM and only the 2 nt ne + 2 doubles of the histogram come back (include/kr_trace.h,
// kr_line_bins, has the per-ray rules).
//
// Reads the parameter file of kr_imageplane_disc_image and the plane and disc keys of imageplane_app.h (--parfile, outfile, dist, incl, plane_phi0, spin,
// r_disc, x0, xmax, Nx, y0, ymax, Ny, img_Nx, img_Ny, q1, rb1, q2, rb2, q3, precision, flip_image, integrator, rk45_tol; --arithmetic, --device, --timing), and
//   line_en = 6.4            rest-frame line energy
//   e_min = 1, e_max = 10    energy range; ne = 90 bins, or de = the bin width (the ratio between edges with log_e = 1)
//   log_e = 0                logarithmic energy bins
//   nt = 1, t0 = 0, dt = 0   time bins of tau = t (+ the table's source->disc time) - t0; dt <= 0 with nt = 1: no time axis
//   g_index = 3              weight = emissivity * g^-g_index
//   line_mode = rays         rays: every ray that reaches the disc; pixels: the notebook's per-pixel form over the img_Nx x img_Ny image
//   emis_file                optional 7-column emissivity table (kr_emissivity / the reference's emissivity: r, area, rays, flux, emis,
//                            redshift, time) used instead of powerlaw3: its emis column and its time column (the source->disc delay);
//                            the r column must be log-spaced
//   limb, limb_coeff = 2.06  optional limb law of the emission angle mu in the disc frame (line_mode = rays): 0 isotropic, 1 the weight
//                            1 + limb_coeff mu (Laor), 2 log(1 + 1 / mu) (limb brightening); kr_limb_law in include/kr_trace.h
//   disc_slope, disc_scale   (and disc_rin = ISCO; imageplane_app.h, DiscSurfaceKeys) with either key the disc has the surface of KR_STOP_THICKDISC: the
//                            rays stop on it and the line is that of the rays that landed on it, binned by the cylindrical radius rho, the limb law
//                            taken to the surface normal (kr_post_line_surface_dev_f64; line_mode = rays, no plunge); the file opens with the rows
//                            "# DISCSLOP", "# DISCSCAL", "# DISCRIN".  Without the keys the program and its file are what they were.
// Every key may also be given as --key=value, which takes precedence over the file.  Nx, Ny, img_Nx and img_Ny are read as int, as
// kr_imageplane_disc_image reads them (before imageplane_app.h: as double, then cast; the same for a key written as a plain integer).
// Output: TextOutput (width 20, precision 8), one row per bin: t_mid E_mid flux count (t_mid is nan without a time axis), a blank line
// after each time bin.  With `limb` given two comment rows "# LIMB" and "# LIMBCOEF" with their values come first; without it the file is
// what it was before the key existed.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/text_output.h"
#include "emissivity_table.h"
#include "imageplane_app.h"

static void program(const krapp::Options& opt)
{
    const krapp::DiscPlaneSetup s(opt, true);
    const double line_en = opt.num("line_en", 6.4), e_min = opt.num("e_min", 1), e_max = opt.num("e_max", 10), g_index = opt.num("g_index", 3);
    const bool log_e = opt.num("log_e", 0) != 0;
    int ne;
    double de;
    if (opt.has("de") && !opt.has("ne")) {
        de = opt.req("de");
        ne = (int) lround(log_e ? log(e_max / e_min) / log(de) : (e_max - e_min) / de);
    } else {
        ne = (int) opt.num("ne", 90);
        de = log_e ? exp(log(e_max / e_min) / ne) : (e_max - e_min) / ne;
    }
    const int nt = (int) opt.num("nt", 1);
    const double t0 = opt.num("t0", 0), dt = opt.num("dt", 0);
    const string mode = opt.str("line_mode", "rays");
    if (mode != "rays" && mode != "pixels") throw invalid_argument("line_mode: expected rays or pixels, got '" + mode + "'");
    const string emis_file = opt.str("emis_file", "");
    const bool with_limb = opt.has("limb");
    kr_limb_law limb;
    memset(&limb, 0, sizeof limb);
    limb.law = (int32_t) opt.num("limb", 0);
    limb.coeff = opt.num("limb_coeff", 2.06);
    if (with_limb && mode != "rays") throw invalid_argument("limb: a limb law needs line_mode = rays (a pixel's mean has no emission angle)");
    const krapp::DiscSurfaceKeys disc(opt, s.r_isco, s.r_disc);
    disc.refuse_with(s.flow.plunge, opt.has("pol_law") || opt.has("pol_coeff"));
    if (disc.thick && mode != "rays") throw invalid_argument("disc_slope / disc_scale: the line of a disc surface needs line_mode = rays");
    s.print_isco();

    const kr_imageplane plane = s.plane();
    kr_line_bins lb;
    memset(&lb, 0, sizeof lb);
    lb.line_energy = line_en;
    lb.e_min = e_min; lb.de = de; lb.ne = ne; lb.log_e = log_e ? 1 : 0;
    lb.t0 = t0; lb.dt = dt; lb.nt = nt;
    s.fill_disc(lb);
    lb.g_index = g_index;
    krapp::EmisTable table;
    if (!emis_file.empty()) {
        table = krapp::read_emis_table(emis_file);
        lb.table_r_min = table.r_min; lb.table_dr = table.dr; lb.table_logbin = 1;
        lb.table_nr = (int32_t) table.emis.size();
        lb.table_emis = table.emis.data();
        lb.table_time = table.time.data();
        cout << "emissivity table " << emis_file << ": " << lb.table_nr << " bins from r = " << table.r_min << ", ratio " << table.dr << endl;
    }

    const kr_image_bins ib = s.image_bins();
    kr_params p = s.params(KR_RK45);
    disc.stop_on(p);

    // ---- device pipeline: init_emit -> trace -> (redshift + range_phi + line) or (redshift + range_phi + planes -> line) ----------------
    krapp::DiscPlaneRun run(s, plane);
    const bool with_angle = with_limb || disc.thick;
    const int64_t words = 2 * (int64_t) nt * ne + 2 + (with_angle ? 1 : 0);      // the limb and surface passes close their histogram with bad_angle
    run.trace(plane, p, words);
    void *rays = run.rays->get(), *line = run.acc->get();
    if (disc.thick) {
        krapp::check(kr_post_line_surface_dev_f64(&disc.surface, -s.spin, 1, -1 * M_PI, M_PI, &lb, &limb, rays, run.n, line, nullptr), "redshift + range_phi + line of the surface");
    } else if (with_limb) {
        krapp::check(kr_post_line_limb_dev_f64(-s.spin, s.flow.V(), 1, 0, 0, -1 * M_PI, M_PI, &lb, &limb, rays, run.n, line, nullptr), "redshift + range_phi + limb-law line");
    } else if (mode == "rays") {
        krapp::check(kr_post_line_dev_f64(-s.spin, s.flow.V(), 1, 0, 0, -1 * M_PI, M_PI, &lb, rays, run.n, line, nullptr), "redshift + range_phi + line");
    } else {
        const int64_t npix = (int64_t) ib.img_nx * ib.img_ny;
        krapp::DeviceBuffer planes((7 * npix + 1) * (int64_t) sizeof(double));
        planes.zero();
        krapp::check(kr_post_image_dev_f64(-s.spin, s.flow.V(), 1, 0, 0, -1 * M_PI, M_PI, &ib, rays, run.n, planes.get(), nullptr), "redshift + range_phi + image planes");
        krapp::check(kr_line_from_image_dev_f64(&lb, &ib, planes.get(), line, nullptr), "line from image planes");
        krapp::check(kr_synchronize(nullptr), "sync");
    }
    vector<double> h((size_t) words);
    krapp::check(kr_memcpy_d2h(h.data(), line, words * (int64_t) sizeof(double)), "d2h");
    const double ms_post = run.clock.lap_ms();

    const int64_t nb = (int64_t) nt * ne;
    cout << static_cast<long>(h[nb * 2]) << (mode == "rays" ? " rays" : " pixels") << " on the disc, " << static_cast<long>(h[nb * 2 + 1]) << " binned" << endl;
    if (with_angle) cout << static_cast<long>(h[nb * 2 + 2]) << " rays on the disc have no emission angle (bad-angle)" << endl;
    {
        TextOutput outfile(s.out_name);
        s.flow.write_rows(outfile);
        disc.write_rows(outfile);
        if (with_limb) {
            outfile << "# LIMB" << limb.law << endl;
            outfile << "# LIMBCOEF" << limb.coeff << endl;
        }
        const bool time_axis = !(nt == 1 && dt <= 0);
        for (int j = 0; j < nt; ++j) {
            const double t_mid = time_axis ? t0 + (j + 0.5) * dt : NAN;
            for (int i = 0; i < ne; ++i) {
                const double lo = log_e ? e_min * pow(de, i) : e_min + i * de, hi = log_e ? e_min * pow(de, i + 1) : e_min + (i + 1) * de;
                outfile << t_mid << 0.5 * (lo + hi) << h[nb + (int64_t) j * ne + i] << static_cast<long>(h[(int64_t) j * ne + i]) << endl;
            }
            outfile << endl;
        }
    }
    const double ms_out = run.clock.lap_ms();

    if (s.timing)
        run.print_timing() << (mode == "rays" ? "redshift+range_phi+line" : "redshift+range_phi+planes+line") << "+readback " << ms_post << " ms | text file " << ms_out << " ms"
                           << endl;
}

int main(int argc, char** argv) { return krapp::run_program(argc, argv, "../par/imageplane_disc_image.par", program); }
