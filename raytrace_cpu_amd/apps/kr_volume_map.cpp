// apps/kr_volume_map.cpp -- what a point source illuminates between itself and the disc: the rays of a PointSource are generated and traced on the
// MI355X and binned into an (r, theta, phi) grid AS THEY STEP (kr_trace_volume_dev_f64; include/kr_trace.h has the rule), with their arrival time and
// energy shift.  This is Mapper_PointSource + Mapper::run_map + average_rays + save_hdf of the reference (src/mapper/), whose own text sits on an API
// that no longer exists: the rule is restated against the live trace loop, and the file is FITS from this tree's writer instead of HDF5.
//
// Reads: --parfile (default ../par/volume_map.par), --outfile | outfile, source[4], V = 0 (the source's angular velocity: redshift_start), --spin | spin,
// cosalpha0 = -0.995, cosalphamax = 0.995, dcosalpha, beta0 = -pi, betamax = pi, dbeta, r0 (first radial edge), rmax, Nr, Ntheta, Nphi = 1,
// logbin_r = false, theta_max = pi / 2 and r_esc = 1000 (where the trace stops), --integrator | integrator = rk4 (euler | rk4), mode = 0 (0: one deposit
// per passage of a cell, 1: one per step -- the reference's literal behaviour), --source_h, --device = 0, --timing.
// The grid has the bin widths of Mapper's constructor (mapper.cpp:14-16: n - 1 divisions of [r0, rmax], [0, pi / 2], [0, 2 pi]; an axis of one cell
// spans the whole range); the energy shift is measured by the mapper's observers, on orbits of V = 1 / (a + r sin(theta) sqrt(r sin(theta))).
//
// outfile: a FITS file with four image extensions of NAXIS1 = Ntheta * Nphi by NAXIS2 = Nr pixels, pixel [ir][itheta * Nphi + iphi] like Array3D:
// NRAYS (deposits), TIME and REDSHIFT (their means per deposit, as average_rays leaves them: 0 / 0 = NaN where nothing crossed) and VOLUME
// (calculate_volume, mapper.cpp:311-338).  The primary header carries the attributes save_hdf writes (r0, rmax, Nr, dr, logbin_r, theta_max, Ntheta,
// dtheta, Nphi, dphi), spin, mode, num_rays and the four tallies rows / in_grid / deposits / bad_g.
#include <algorithm>
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/fits_output.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "app_common.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();
    ParameterArgs args(argc, argv);
    const string par_name = args.key_exists("--parfile") ? args.get_string_parameter("--parfile") : string("../par/volume_map.par");
    ParameterFile par(par_name);

    const string out_name = args.key_exists("--outfile") ? args.get_parameter<string>("--outfile") : par.get_parameter<string>("outfile");
    double source[4];
    par.get_parameter_array("source", source, 4);
    if (args.key_exists("--source_h")) source[1] = args.get_parameter<double>("--source_h");
    const double V = par.get_parameter<double>("V", 0);
    const double spin = args.key_exists("--spin") ? args.get_parameter<double>("--spin") : par.get_parameter<double>("spin");
    const double r0 = par.get_parameter<double>("r0");
    const double rmax = par.get_parameter<double>("rmax");
    const int Nr = par.get_parameter<int>("Nr");
    const int Ntheta = par.get_parameter<int>("Ntheta");
    const int Nphi = par.get_parameter<int>("Nphi", 1);
    const bool logbin_r = par.get_parameter<bool>("logbin_r", false);
    const double theta_max = par.get_parameter<double>("theta_max", M_PI_2);
    const double r_esc = par.get_parameter<double>("r_esc", 1000);
    const int mode = par.get_parameter<int>("mode", 0);
    const string integ = args.key_exists("--integrator") ? args.get_parameter<string>("--integrator") : par.get_parameter<string>("integrator", "rk4");
    const bool timing = args.key_exists("--timing");
    if (Nr < 1 || Ntheta < 1 || Nphi < 1) throw runtime_error("Nr, Ntheta and Nphi must be at least 1");

    kr_pointsource src;
    memset(&src, 0, sizeof src);
    for (int i = 0; i < 4; ++i) src.pos[i] = source[i];
    src.V = V; src.spin = spin; src.tol = 100; src.E = 1;
    src.cosalpha0 = par.get_parameter<double>("cosalpha0", -0.995);
    src.cosalphamax = par.get_parameter<double>("cosalphamax", 0.995);
    src.dcosalpha = par.get_parameter<double>("dcosalpha");
    src.beta0 = par.get_parameter<double>("beta0", -1 * M_PI);
    src.betamax = par.get_parameter<double>("betamax", M_PI);
    src.dbeta = par.get_parameter<double>("dbeta");

    // Mapper's constructor, mapper.cpp:14-16
    kr_volume_map m;
    memset(&m, 0, sizeof m);
    m.r_min = r0;
    m.dr = logbin_r ? exp(log(rmax / r0) / max(Nr - 1, 1)) : (rmax - r0) / max(Nr - 1, 1);
    m.dtheta = (M_PI_2) / max(Ntheta - 1, 1);
    m.dphi = (2 * M_PI) / max(Nphi - 1, 1);
    m.V = -1; m.projradius = 1; m.reverse = 0; m.motion = 0;
    m.nr = Nr; m.ntheta = Ntheta; m.nphi = Nphi; m.logbin = logbin_r ? 1 : 0; m.mode = mode;

    kr_params p;
    kr_params_default(&p, spin);
    p.integrator = krapp::integrator_code(integ, KR_RK4);
    p.theta_max = theta_max;
    p.r_max = r_esc;
    p.stop_kind = KR_STOP_THETA;
    p.flags = 0;                         // the map rides the strict recording loop

    krapp::require_device();             // before the output file is created
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch clock;
    const int64_t n = kr_pointsource_count(&src, nullptr, nullptr);
    if (n <= 0) throw runtime_error("empty ray grid");
    const int64_t ncell = (int64_t) Nr * Ntheta * Nphi, words = 3 * ncell + 4;
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    krapp::DeviceBuffer map(words * (int64_t) sizeof(double));
    map.zero();
    krapp::check(kr_pointsource_init_emit_dev_f64(&src, 0, 1, V, 0, 0, rays.get(), n, nullptr), "pointsource_init + redshift_start");
    kr_stats st;
    krapp::check(kr_trace_volume_dev_f64(&p, &m, rays.get(), n, map.get(), nullptr, &st), "volume map");
    vector<double> h(static_cast<size_t>(words));
    krapp::check(kr_memcpy_d2h(h.data(), map.get(), words * (int64_t) sizeof(double)), "d2h");
    const double ms_device = clock.lap_ms();

    // average_rays (mapper.cpp:304-308) and calculate_volume (:311-338)
    vector<double> mean_time(static_cast<size_t>(ncell)), mean_g(static_cast<size_t>(ncell)), volume(static_cast<size_t>(ncell));
    for (int64_t c = 0; c < ncell; ++c) {
        mean_time[c] = h[ncell + c] / h[c];
        mean_g[c] = h[2 * ncell + c] / h[c];
    }
    for (int ir = 0; ir < Nr; ++ir) {
        const double a = spin;
        const double r = logbin_r ? r0 * pow(m.dr, ir) : r0 + m.dr * ir;
        const double this_bin_dr = logbin_r ? r * (m.dr - 1) : m.dr;
        for (int itheta = 0; itheta < Ntheta; ++itheta) {
            const double theta = itheta * m.dtheta;
            const double rhosq = r * r + (a * cos(theta)) * (a * cos(theta));
            const double delta = r * r - 2 * r + a * a;
            const double sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * sin(theta) * sin(theta);
            const double e2psi = sigmasq * sin(theta) * sin(theta) / rhosq;
            const double grr = -rhosq / delta, gthth = -rhosq, gphph = -e2psi;
            for (int iphi = 0; iphi < Nphi; ++iphi)
                volume[((size_t) ir * Ntheta + itheta) * Nphi + iphi] = sqrt(-1 * grr * gthth * gphph) * this_bin_dr * m.dtheta * m.dphi;
        }
    }

    FITSOutput<double> fits(out_name);
    fits.create_primary();
    fits.write_comment("Kerr BH volume illumination map of a point source");
    fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "kr_volume_map");
    fits.write_keyword("SPIN", "Black hole spin parameter a/M", spin);
    fits.write_keyword("R0", "First radial edge (rg)", r0);
    fits.write_keyword("RMAX", "Lower edge of the last radial cell (rg)", rmax);
    fits.write_keyword("NR", "Radial cells", Nr);
    fits.write_keyword("DR", "Cell width (rg), or ratio between edges with LOGBIN_R", m.dr);
    fits.write_keyword("LOGBIN_R", "1 = logarithmic radial cells", logbin_r ? 1 : 0);
    fits.write_keyword("THETAMAX", "Polar angle at which the trace stops", theta_max);
    fits.write_keyword("NTHETA", "Polar cells, from theta = 0", Ntheta);
    fits.write_keyword("DTHETA", "Polar cell width", m.dtheta);
    fits.write_keyword("NPHI", "Azimuthal cells, from phi = -pi", Nphi);
    fits.write_keyword("DPHI", "Azimuthal cell width", m.dphi);
    fits.write_keyword("MODE", "0 = one deposit per passage of a cell, 1 = per step", mode);
    fits.write_keyword("NUM_RAYS", "Rays traced", (long) st.rays_traced);
    fits.write_keyword("ROWS", "Ray steps that could deposit", (long) llround(h[3 * ncell]));
    fits.write_keyword("IN_GRID", "... of them inside the grid", (long) llround(h[3 * ncell + 1]));
    fits.write_keyword("DEPOSITS", "Deposits: the sum of NRAYS", (long) llround(h[3 * ncell + 2]));
    fits.write_keyword("BAD_G", "Due deposits dropped for g <= 0 or not finite", (long) llround(h[3 * ncell + 3]));
    const char* names[4] = {"NRAYS", "TIME", "REDSHIFT", "VOLUME"};
    const char* what[4] = {"Deposits per cell", "Mean coordinate time of arrival per deposit", "Mean energy shift g per deposit",
                           "Proper volume of the cell, sqrt(-g_rr g_thth g_phph) dr dtheta dphi at its lower corner"};
    double* planes[4] = {h.data(), mean_time.data(), mean_g.data(), volume.data()};
    for (int k = 0; k < 4; ++k) {
        fits.write_image_array(planes[k], Ntheta * Nphi, Nr);
        fits.set_ext_name(names[k]);
        fits.write_comment(what[k]);
        fits.write_comment("pixel [ir][itheta * NPHI + iphi]; cells no ray crossed are NaN in TIME and REDSHIFT");
    }
    fits.close();

    if (timing)
        cout << "timing: rays " << st.rays_traced << " steps " << st.steps_total << " cells " << ncell << " | init + map " << ms_device << " ms (map launch " << st.kernel_ms
             << ") | files " << clock.lap_ms() << " ms" << endl;
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
