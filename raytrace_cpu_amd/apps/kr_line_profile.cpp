// apps/kr_line_profile.cpp -- the relativistically broadened emission line (and, with a time axis, the reverberation transfer function) of
// the disc seen on an image plane, resident on the MI355X from start to finish.  The reference builds the line outside its C++: it writes the
// image FITS file with imageplane_disc_image and sums ENSHIFT / RADIUS pixels into energy bins in python/line_from_image.ipynb.  Here the rays
// are generated, traced, redshifted and binned in HBM and only the 2 nt ne + 2 doubles of the histogram come back (include/kr_trace.h,
// kr_line_bins, has the per-ray rules).
//
// Reads the parameter file and keys of kr_imageplane_disc_image (--parfile, outfile, dist, incl, plane_phi0, spin, r_disc, x0, xmax, Nx, y0,
// ymax, Ny, img_Nx, img_Ny, q1, rb1, q2, rb2, q3, precision, flip_image, integrator, rk45_tol; --arithmetic, --device, --timing), and
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
// Every key may also be given as --key=value, which takes precedence over the file.
// Output: TextOutput (width 20, precision 8), one row per bin: t_mid E_mid flux count (t_mid is nan without a time axis), a blank line
// after each time bin.  With `limb` given two comment rows "# LIMB" and "# LIMBCOEF" with their values come first; without it the file is
// what it was before the key existed.
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/kerr.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "../host/include/text_output.h"
#include "app_common.h"
#include "emissivity_table.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();       // first HIP user of this process (include/kr_trace.h)
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/imageplane_disc_image.par");
    ParameterFile par(par_name);
    // --key=value first, then the parameter file, then the default
    auto num = [&](const string& key, double dflt) { return args.key_exists("--" + key) ? args.get_parameter<double>("--" + key) : par.get_parameter<double>(key, dflt); };
    auto req = [&](const string& key) { return args.key_exists("--" + key) ? args.get_parameter<double>("--" + key) : par.get_parameter<double>(key); };
    auto has = [&](const string& key) { return args.key_exists("--" + key) || par.key_exists(key); };
    auto str = [&](const string& key, const string& dflt) { return args.key_exists("--" + key) ? args.get_parameter<string>("--" + key) : par.get_parameter<string>(key, dflt); };

    const string out_name = args.key_exists("--outfile") ? args.get_parameter<string>("--outfile") : par.get_parameter<string>("outfile");
    const double dist = req("dist"), incl = req("incl"), plane_phi0 = num("plane_phi0", 0), spin = req("spin"), r_disc = req("r_disc");
    const double x0 = num("x0", -1 * r_disc), xmax = num("xmax", r_disc);
    const int Nx = (int) req("Nx");
    const double y0 = num("y0", x0), ymax = num("ymax", xmax);
    const int Ny = (int) num("Ny", Nx);
    const int img_nx = (int) num("img_Nx", Nx), img_ny = (int) num("img_Ny", img_nx);
    const double q1 = num("q1", 3), rb1 = num("rb1", 4), q2 = num("q2", 3), rb2 = num("rb2", 10), q3 = num("q3", 3);
    const double precision = num("precision", 100);
    const bool flip_image = args.key_exists("--flip_image") ? args.get_parameter<bool>("--flip_image") : par.get_parameter<bool>("flip_image", true);
    const string integ = str("integrator", "rk45");
    const double rk45_tol = num("rk45_tol", 1e-8);
    const string arith = args.key_exists("--arithmetic") ? args.get_parameter<string>("--arithmetic") : krapp::arithmetic_from_env();
    const bool timing = args.key_exists("--timing");

    const double line_en = num("line_en", 6.4), e_min = num("e_min", 1), e_max = num("e_max", 10), g_index = num("g_index", 3);
    const bool log_e = num("log_e", 0) != 0;
    int ne;
    double de;
    if (has("de") && !has("ne")) {
        de = req("de");
        ne = (int) lround(log_e ? log(e_max / e_min) / log(de) : (e_max - e_min) / de);
    } else {
        ne = (int) num("ne", 90);
        de = log_e ? exp(log(e_max / e_min) / ne) : (e_max - e_min) / ne;
    }
    const int nt = (int) num("nt", 1);
    const double t0 = num("t0", 0), dt = num("dt", 0);
    const string mode = str("line_mode", "rays");
    if (mode != "rays" && mode != "pixels") throw invalid_argument("line_mode: expected rays or pixels, got '" + mode + "'");
    const string emis_file = str("emis_file", "");
    const bool with_limb = has("limb");
    kr_limb_law limb;
    memset(&limb, 0, sizeof limb);
    limb.law = (int32_t) num("limb", 0);
    limb.coeff = num("limb_coeff", 2.06);
    if (with_limb && mode != "rays") throw invalid_argument("limb: a limb law needs line_mode = rays (a pixel's mean has no emission angle)");

    const double dx = (xmax - x0) / Nx, dy = (ymax - y0) / Ny;
    const double r_isco = kerr_isco<double>(spin, +1);
    cout << "ISCO at " << r_isco << endl;

    kr_imageplane plane;
    memset(&plane, 0, sizeof plane);
    plane.dist = dist;
    plane.inc_deg = incl;
    plane.x0 = x0; plane.xmax = xmax; plane.dx = dx;
    plane.y0 = y0; plane.ymax = ymax; plane.dy = dy;
    plane.spin = spin;
    plane.phi0 = plane_phi0;
    plane.precision = precision;

    kr_line_bins lb;
    memset(&lb, 0, sizeof lb);
    lb.line_energy = line_en;
    lb.e_min = e_min; lb.de = de; lb.ne = ne; lb.log_e = log_e ? 1 : 0;
    lb.t0 = t0; lb.dt = dt; lb.nt = nt;
    lb.r_isco = r_isco; lb.r_disc = r_disc;
    lb.q1 = q1; lb.rb1 = rb1; lb.q2 = q2; lb.rb2 = rb2; lb.q3 = q3;
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

    kr_image_bins ib;
    memset(&ib, 0, sizeof ib);
    ib.x0 = x0; ib.y0 = y0;
    ib.img_dx = (xmax - x0) / img_nx;
    ib.img_dy = (ymax - y0) / img_ny;
    ib.r_isco = r_isco; ib.r_disc = r_disc;
    ib.q1 = q1; ib.rb1 = rb1; ib.q2 = q2; ib.rb2 = rb2; ib.q3 = q3;
    ib.img_nx = img_nx; ib.img_ny = img_ny;
    ib.flip_image = flip_image ? 1 : 0;

    kr_params p;
    kr_params_default(&p, -spin);            // the image plane traces backwards in time: spin enters negated (imageplane.cpp:12)
    p.precision = precision;
    p.integrator = krapp::integrator_code(integ, KR_RK45);
    if (p.integrator == KR_RK45) p.rk45_tol = rk45_tol;
    p.theta_max = M_PI_2;
    p.r_max = 1.1 * dist;
    p.stop_kind = KR_STOP_THETA;
    p.flags = krapp::arithmetic_flags(arith, p.integrator);

    // ---- device pipeline: init_emit -> trace -> (redshift + range_phi + line) or (redshift + range_phi + planes -> line) ----------------
    krapp::check(kr_set_device((int) num("device", 0)), "kr_set_device");
    krapp::Stopwatch clock;
    const int64_t n = kr_imageplane_count(&plane, nullptr, nullptr);
    if (n <= 0) throw runtime_error("empty ray grid");
    const int64_t words = 2 * (int64_t) nt * ne + 2 + (with_limb ? 1 : 0);      // the limb pass closes its histogram with bad_angle
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    krapp::DeviceBuffer line(words * (int64_t) sizeof(double));
    line.zero();
    krapp::check(kr_imageplane_init_emit_dev_f64(&plane, 0, 1, 0.0, 1, 0, rays.get(), n, nullptr), "imageplane_init + redshift_start");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_init = clock.lap_ms();
    kr_stats st;
    krapp::check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &st), "trace");
    const double ms_trace = clock.lap_ms();
    if (with_limb) {
        krapp::check(kr_post_line_limb_dev_f64(-spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, &lb, &limb, rays.get(), n, line.get(), nullptr), "redshift + range_phi + limb-law line");
    } else if (mode == "rays") {
        krapp::check(kr_post_line_dev_f64(-spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, &lb, rays.get(), n, line.get(), nullptr), "redshift + range_phi + line");
    } else {
        const int64_t npix = (int64_t) img_nx * img_ny;
        krapp::DeviceBuffer planes((7 * npix + 1) * (int64_t) sizeof(double));
        planes.zero();
        krapp::check(kr_post_image_dev_f64(-spin, -1.0, 1, 0, 0, -1 * M_PI, M_PI, &ib, rays.get(), n, planes.get(), nullptr), "redshift + range_phi + image planes");
        krapp::check(kr_line_from_image_dev_f64(&lb, &ib, planes.get(), line.get(), nullptr), "line from image planes");
        krapp::check(kr_synchronize(nullptr), "sync");
    }
    vector<double> h((size_t) words);
    krapp::check(kr_memcpy_d2h(h.data(), line.get(), words * (int64_t) sizeof(double)), "d2h");
    const double ms_post = clock.lap_ms();

    const int64_t nb = (int64_t) nt * ne;
    cout << static_cast<long>(h[nb * 2]) << (mode == "rays" ? " rays" : " pixels") << " on the disc, " << static_cast<long>(h[nb * 2 + 1]) << " binned" << endl;
    if (with_limb) cout << static_cast<long>(h[nb * 2 + 2]) << " rays on the disc have no emission angle (bad-angle)" << endl;
    {
        TextOutput outfile(out_name);
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
    const double ms_out = clock.lap_ms();

    if (timing)
        cout << "timing: rays " << st.rays_traced << " steps " << st.steps_total << " | init+redshift_start " << ms_init << " ms | trace " << ms_trace
             << " ms (kernel " << st.kernel_ms << ") | " << (mode == "rays" ? "redshift+range_phi+line" : "redshift+range_phi+planes+line") << "+readback "
             << ms_post << " ms | text file " << ms_out << " ms" << endl;
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
