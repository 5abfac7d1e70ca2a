// apps/kr_angdist.cpp -- the reference's disc_source_return_angdist program (src/return_radiation/disc_source_return_angdist.cpp; stale there: it calls
// accessors that no longer exist) resident on the MI355X, and the same question for an emitter with ANY four-velocity: into which directions of its own
// sky a source sends the light that returns to the disc, escapes or is lost to the hole.  Source -> trace -> range_phi + redshift + the histograms
// (kr_post_angdist_dev_f64) without a ray record leaving the device; only the 14 Nangle + 8 words come back.
//
// Reads (:37-58): --parfile (default ../par/disc_source_return_angdist.par), --outfile | outfile, --source_r | source_r, source_phi = 1.5707, V = -1
// (negative: the disc's velocity at source_r, :110), --spin | spin, cosalpha0 = -0.995, cosalphamax = 0.995, dcosalpha, beta0 = -pi, betamax = pi, dbeta,
// show_progress = 1, r_esc = 1000, plane_iso = 1, limb = 0, weight_norm = 1, dangle = 0.1.  r_disc := the r_esc key with default 500 (sic, :54); the
// explicit key r_disc, an extension, overrides it.
// With source_r the source is the reference's: a PointSource at (0, source_r, pi/2 - 1e-6, source_phi) on the orbit of angular velocity V, sampled over
// beta from 0 to pi whatever beta0 / betamax say (:117-123: the half of its sky above the disc), the histograms in PointSource's labels (labels = 0).
// Extensions: without source_r,  source = t r theta phi  places an emitter anywhere, with  velocity = ut ur utheta uphi  (need not be normalised) or the
// coordinate velocities  omega  (default: the frame dragging rate, -g_tphi / g_phiphi)  dr_dt = 0  dtheta_dt = 0;  that source is the PointSourceVel
// (kr_pointsource_vel_init_emit_dev_f64) over beta0 ... betamax, and the histograms read its labels (labels = 1).  self_zone = 0 | 1 (default 0, as the
// reference has the test commented out, :161): rays that land within 0.1 source_r and 0.1 rad of the source count as neither returned nor lost.
// integrator = euler (:126), --arithmetic | KRTRACE_ARITHMETIC, --device = 0, --timing.
//
// Writes the reference's 13 columns (:216-222): angle = -pi + i dangle, then alpha, beta, norm, az of escape, return, lost; the three az columns divided
// by their sum per bin (:200-209; an empty bin is 0 / 0 as there).  Prints Escape, Return, Lost over the ray count (:211-213).
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

int main(int argc, char** argv)
try {
    (void) kr_configure_process();
    const krapp::Options opt(argc, argv, "../par/disc_source_return_angdist.par");
    const ParameterArgs& args = opt.args;
    const ParameterFile& par = opt.par;

    const string out_filename = opt.str("outfile");
    const bool disc_source = opt.has("source_r");
    const double spin = opt.req("spin");
    const double cosalpha0 = par.get_parameter<double>("cosalpha0", -0.995);
    const double cosalphamax = par.get_parameter<double>("cosalphamax", 0.995);
    const double dcosalpha = par.get_parameter<double>("dcosalpha");
    const double beta0 = par.get_parameter<double>("beta0", -1 * M_PI);
    const double betamax = par.get_parameter<double>("betamax", M_PI);
    const double dbeta = par.get_parameter<double>("dbeta");
    const int show_progress = par.get_parameter<int>("show_progress", 1);
    const double r_esc = par.get_parameter<double>("r_esc", 1000);
    const double r_disc = par.key_exists("r_disc") ? par.get_parameter<double>("r_disc") : par.get_parameter<double>("r_esc", 500);
    const bool plane_iso = par.get_parameter<bool>("plane_iso", true);
    const bool limb = par.get_parameter<bool>("limb", false);
    const bool weight_norm = par.get_parameter<bool>("weight_norm", true);
    const double dangle = par.get_parameter<double>("dangle", 0.1);
    const bool self_zone = par.get_parameter<bool>("self_zone", false);
    const string integ = par.get_parameter<string>("integrator", "euler");
    const string arith = krapp::arithmetic_choice(opt);
    const bool timing = opt.on_command_line("timing");

    kr_pointsource ps;
    kr_pointsource_vel_spec vs;
    memset(&ps, 0, sizeof ps);
    memset(&vs, 0, sizeof vs);
    double source[4];
    int64_t n = 0;
    if (disc_source) {
        const double source_r = opt.req("source_r");
        double V = par.get_parameter<double>("V", -1);
        if (V < 0) V = disc_velocity<double>(source_r, spin, +1);
        source[0] = 0.; source[1] = source_r; source[2] = M_PI_2 - 1E-6; source[3] = par.get_parameter<double>("source_phi", 1.5707);
        for (int i = 0; i < 4; i++) ps.pos[i] = source[i];
        ps.V = V; ps.spin = spin; ps.tol = 100; ps.E = 1;
        ps.dcosalpha = dcosalpha; ps.dbeta = dbeta; ps.cosalpha0 = cosalpha0; ps.cosalphamax = cosalphamax;
        ps.beta0 = 0; ps.betamax = M_PI;
        cout << "beta = " << ps.beta0 << " to " << ps.betamax << endl;
        n = kr_pointsource_count(&ps, nullptr, nullptr);
    } else {
        par.get_parameter_array<double>("source", source, 4);
        for (int i = 0; i < 4; i++) vs.pos[i] = source[i];
        if (par.key_exists("velocity")) {
            par.get_parameter_array<double>("velocity", vs.u, 4);
        } else {
            // u = (1, dr/dt, dtheta/dt, omega): the library normalises it and refuses one that is not timelike
            const double r = source[1], st = sin(source[2]);
            const double delta = r * r - 2 * r + spin * spin;
            const double sigmasq = (r * r + spin * spin) * (r * r + spin * spin) - spin * spin * delta * st * st;
            vs.u[0] = 1;
            vs.u[1] = par.get_parameter<double>("dr_dt", 0);
            vs.u[2] = par.get_parameter<double>("dtheta_dt", 0);
            vs.u[3] = par.get_parameter<double>("omega", 2 * spin * r / sigmasq);
        }
        vs.spin = spin; vs.tol = 100; vs.E = 1;
        vs.dcosalpha = dcosalpha; vs.dbeta = dbeta; vs.cosalpha0 = cosalpha0; vs.cosalphamax = cosalphamax; vs.beta0 = beta0; vs.betamax = betamax;
        n = kr_pointsource_vel_count(&vs, nullptr, nullptr);
        if (n < 0) throw runtime_error(kr_last_error());
    }

    kr_angdist_spec sp;
    memset(&sp, 0, sizeof sp);
    sp.cls.r_isco = kerr_isco<double>(spin, +1);
    sp.cls.r_disc = r_disc; sp.cls.r_esc = r_esc;
    sp.cls.source_r = self_zone ? source[1] : 0; sp.cls.source_phi = source[3];
    sp.cls.plane_iso = plane_iso; sp.cls.limb = limb; sp.cls.weight_norm = weight_norm;
    sp.dangle = dangle;
    sp.labels = disc_source ? 0 : 1;
    const int Nangle = kr_angdist_nangle(&sp);
    if (Nangle < 0) throw runtime_error(kr_last_error());

    kr_params p;
    kr_params_default(&p, spin);
    p.integrator = krapp::integrator_code(integ, KR_EULER);
    p.theta_max = M_PI_2;
    p.r_max = 1.1 * r_esc;
    p.stop_kind = KR_STOP_THETA;
    p.flags = krapp::arithmetic_flags(arith, p.integrator);

    krapp::require_device();
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch wall, clock;
    const int64_t words = 14 * (int64_t) Nangle + 8;
    krapp::DeviceBuffer rays((n > 0 ? n : 1) * (int64_t) sizeof(kr_ray_f64));
    krapp::DeviceBuffer out(words * (int64_t) sizeof(double));
    out.zero();
    if (disc_source) krapp::check(kr_pointsource_init_emit_dev_f64(&ps, 0, 1, ps.V, 0, 0, rays.get(), n, nullptr), "point source + redshift_start");
    else krapp::check(kr_pointsource_vel_init_emit_dev_f64(&vs, rays.get(), n, nullptr), "point source (four-velocity) + emitted energy");
    double ms_init = 0, ms_trace = 0, ms_post = 0;
    if (timing) { krapp::check(kr_synchronize(nullptr), "sync"); ms_init = clock.lap_ms(); }
    kr_stats stats;
    memset(&stats, 0, sizeof stats);
    if (show_progress > 0) cout << "Tracing " << n << " rays" << endl;
    krapp::check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &stats), "trace");
    if (timing) ms_trace = clock.lap_ms();
    krapp::check(kr_post_angdist_dev_f64(spin, -1.0, 0, 0, 0, -1 * M_PI, M_PI, &sp, rays.get(), n, out.get(), nullptr), "range_phi + redshift + angular distribution");
    vector<double> w((size_t) words);
    krapp::check(kr_memcpy_d2h(w.data(), out.get(), words * (int64_t) sizeof(double)), "d2h");
    if (timing) ms_post = clock.lap_ms();

    // [escape | return | lost] x [alpha | beta | norm | az], then total_norm, total_az and the tallies {ray_count, escape, return, lost, other, skipped, out_of_range, bad_g}
    auto hist = [&](int cls, int angle) { return &w[(size_t) (4 * cls + angle) * (size_t) Nangle]; };
    const double* tally = &w[(size_t) 14 * (size_t) Nangle];
    for (int i = 0; i < Nangle; i++) {
        const double az_dist_sum = hist(0, 3)[i] + hist(1, 3)[i] + hist(2, 3)[i];
        hist(0, 3)[i] /= az_dist_sum;
        hist(1, 3)[i] /= az_dist_sum;
        hist(2, 3)[i] /= az_dist_sum;
    }
    const double ray_count = tally[0];
    cout << endl << "Escape: " << tally[1] / ray_count << endl;
    cout << "Return: " << tally[2] / ray_count << endl;
    cout << "Lost:   " << tally[3] / ray_count << endl << endl;
    if (tally[4] != 0 || tally[5] != 0 || tally[6] != 0)
        cout << "In no class: " << tally[4] << ", skipped (cos alpha = 0): " << tally[5] << ", angles out of range: " << tally[6] << endl;

    TextOutput outfile((char*) out_filename.c_str());
    for (int i = 0; i < Nangle; i++) {
        const double angle = -1 * M_PI + i * dangle;
        outfile << angle;
        for (int cls = 0; cls < 3; cls++)
            for (int a = 0; a < 4; a++) outfile << hist(cls, a)[i];
        outfile << endl;
    }
    outfile.close();
    if (timing)
        cout << "timing: rays " << stats.rays_traced << " steps " << stats.steps_total << " | source " << ms_init << " ms | trace " << ms_trace << " ms (kernels "
             << stats.kernel_ms << ") | range_phi+redshift+histograms " << ms_post << " ms | device total " << wall.lap_ms() << " ms" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
