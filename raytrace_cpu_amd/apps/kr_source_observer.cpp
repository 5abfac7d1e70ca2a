// apps/kr_source_observer.cpp -- the source-to-observer link of a point source, resident on the MI355X: the reference's pointsource_sky program
// (src/lamppost/pointsource_sky.cpp: how much of the source's sky the disc covers) and, of the rays that escape, the direct continuum by observer
// inclination -- its flux, its energy shift and the instant it arrives (include/kr_trace.h, kr_observer_spec).  Source -> trace -> range_phi + redshift
// + the link (kr_post_observer_dev_f64) without a ray record leaving the device; only the Nmu (4 + Nt) + 10 words come back.
//
// Reads the keys of pointsource_sky.par (:46-58): source = t r theta phi, V, spin, cosalpha0 = -0.9999, cosalphamax = 0.9999, dcosalpha, beta0 = -pi,
// betamax = pi, dbeta, r_disc = 400, theta_disc = pi/2, r_max = 1000; each but the four numbers of `source` also as --key=value, like --parfile
// (default ../par/pointsource_sky.par).
// (The reference reads beta0 and betamax and never hands them to its PointSource; here they bound the grid.)
// And: Nmu = 20 bins of cos(theta_obs) from mu0 = 0 in steps of dmu = (1 - mu0) / Nmu; gamma = 0, the photon index of the weight shift^gamma; dist = 0,
// the reference sphere of the arrival time (the image plane's dist; 0: the records' t); t0 = 0, dt, Nt = 0 time rows; r_esc = 0.9 r_max, beyond which a
// ray off the disc has escaped; outfile; integrator = euler, --arithmetic | KRTRACE_ARITHMETIC, --device = 0, show_progress = 1.
//
// Prints the reference's two lines (:95-96) from the tallies: "Total sky" = the source's ray count x dcosalpha dbeta and "Disc" = the class `return` x
// dcosalpha dbeta.  DIFFERS from the reference where a ray meets the plane beyond r_disc: its loop reads r_disc and never tests it (:86).
// Writes the row "# R_f" (return / escape), then per inclination bin: mu (the bin's centre), count, flux (the share of the source's rays in the bin
// over the share of the sphere it covers: 1 for an isotropic source in flat space at gamma = 0), the mean shift, the mean t_ref (nan in an empty bin)
// and, with Nt > 0, the Nt words of the bin's time row; text_output.h's column format.
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
{
    return krapp::run_program(argc, argv, "../par/pointsource_sky.par", [](const krapp::Options& opt) {
        const string out_filename = opt.str("outfile");
        double source[4];
        if (opt.on_command_line("source")) throw invalid_argument("source: give the four numbers in the parameter file");
        opt.par.get_parameter_array<double>("source", source, 4);
        const double V = opt.req("V");
        const double spin = opt.req("spin");
        const double cosalpha0 = opt.num("cosalpha0", -0.9999);
        const double cosalphamax = opt.num("cosalphamax", 0.9999);
        const double dcosalpha = opt.req("dcosalpha");
        const double beta0 = opt.num("beta0", -1 * M_PI);
        const double betamax = opt.num("betamax", M_PI);
        const double dbeta = opt.req("dbeta");
        const double r_disc = opt.num("r_disc", 400);
        const double theta_disc = opt.num("theta_disc", M_PI / 2);
        const double r_max = opt.num("r_max", 1000);
        const double r_esc = opt.num("r_esc", 0.9 * r_max);
        const int Nmu = opt.integer("Nmu", 20);
        const double mu0 = opt.num("mu0", 0);
        const double dmu = opt.num("dmu", (1 - mu0) / Nmu);
        const double gamma = opt.num("gamma", 0);
        const double dist = opt.num("dist", 0);
        const double t0 = opt.num("t0", 0);
        const double dt = opt.num("dt", 0);
        const int Nt = opt.integer("Nt", 0);
        const int show_progress = opt.integer("show_progress", 1);
        const string integ = opt.str("integrator", "euler");
        const string arith = krapp::arithmetic_choice(opt);

        cout << "*****" << endl;
        cout << "Source r = [" << source[0] << " , " << source[1] << " , " << source[2] << " , " << source[3] << "] mu" << endl;
        cout << "Source angular velocity V = " << V << " mu*c" << endl;
        cout << "Spin a = " << spin << endl;
        cout << "*****" << endl << endl;

        kr_pointsource ps;
        memset(&ps, 0, sizeof ps);
        for (int i = 0; i < 4; i++) ps.pos[i] = source[i];
        ps.V = V; ps.spin = spin; ps.tol = 100; ps.E = 1;
        ps.dcosalpha = dcosalpha; ps.dbeta = dbeta; ps.cosalpha0 = cosalpha0; ps.cosalphamax = cosalphamax; ps.beta0 = beta0; ps.betamax = betamax;
        const int64_t n = kr_pointsource_count(&ps, nullptr, nullptr);
        if (n < 0) throw runtime_error("the source's grid gives no ray count");

        kr_observer_spec sp;
        memset(&sp, 0, sizeof sp);
        sp.cls.r_isco = kerr_isco<double>(spin, +1);
        sp.cls.r_disc = r_disc; sp.cls.r_esc = r_esc;
        sp.spin = spin; sp.mu0 = mu0; sp.dmu = dmu; sp.t0 = t0; sp.dt = dt; sp.dist = dist; sp.gamma = gamma; sp.nmu = Nmu; sp.nt = Nt;

        kr_params p;
        kr_params_default(&p, spin);
        p.integrator = krapp::integrator_code(integ, KR_EULER);
        p.theta_max = theta_disc;
        p.r_max = r_max;
        p.stop_kind = KR_STOP_THETA;
        p.flags = krapp::arithmetic_flags(arith, p.integrator);

        krapp::require_device();
        krapp::check(kr_set_device(opt.args.get_parameter<int>("--device", 0)), "kr_set_device");
        // (a spec the pass refuses gets a small buffer: the pass says why before it reads one)
        const bool sized = Nmu >= 1 && Nmu <= 4096 && Nt >= 0 && (int64_t) Nmu * (4 + (int64_t) Nt) <= ((int64_t) 1 << 24);
        const int64_t words = sized ? (int64_t) Nmu * (4 + Nt) + 10 : 10;
        krapp::DeviceBuffer rays((n > 0 ? n : 1) * (int64_t) sizeof(kr_ray_f64));
        krapp::DeviceBuffer out(words * (int64_t) sizeof(double));
        out.zero();
        krapp::check(kr_pointsource_init_emit_dev_f64(&ps, 0, 1, V, 0, 0, rays.get(), n, nullptr), "point source + redshift_start");
        kr_stats stats;
        memset(&stats, 0, sizeof stats);
        if (show_progress > 0) cout << "Tracing " << n << " rays" << endl;
        krapp::check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &stats), "trace");
        krapp::check(kr_post_observer_dev_f64(spin, -1.0, 0, 0, 0, -1 * M_PI, M_PI, &sp, rays.get(), n, out.get(), nullptr), "range_phi + redshift + observer link");
        vector<double> w((size_t) words);
        krapp::check(kr_memcpy_d2h(w.data(), out.get(), words * (int64_t) sizeof(double)), "d2h");

        // [count | sum_w | sum_ws | sum_wt] (Nmu each), the Nmu x Nt rows, then {ray_count, return, escape, lost, other, binned, outside_mu, outside_time, inbound, bad_g}
        const double* tally = &w[(size_t) Nmu * (size_t) (4 + Nt)];
        const double domega = dcosalpha * dbeta;
        const double omega_total = (double) n * domega, omega_disc = tally[1] * domega;
        cout << setw(11) << left << "Total sky: " << setw(10) << omega_total << " (" << omega_total / M_PI << "pi)" << endl;
        cout << setw(11) << left << "Disc: " << setw(10) << omega_disc << " (" << omega_disc / M_PI << "pi)" << endl;
        cout << right << "Return " << tally[1] << ", escape " << tally[2] << ", lost " << tally[3] << ", other " << tally[4] << " of " << tally[0] << " rays; binned " << tally[5]
             << ", outside the inclination bins " << tally[6] << ", outside the time rows " << tally[7] << ", inbound " << tally[8] << ", bad shift " << tally[9] << endl;

        TextOutput outfile((char*) out_filename.c_str());
        outfile << "# R_f" << tally[1] / tally[2] << endl;
        for (int i = 0; i < Nmu; i++) {
            const double sum_w = w[(size_t) Nmu + i];
            const bool any = w[(size_t) i] > 0;
            outfile << mu0 + (i + 0.5) * dmu << (long long) llround(w[(size_t) i]) << (sum_w / tally[0]) / (dmu / 2);
            outfile << (any ? w[(size_t) 2 * Nmu + i] / sum_w : (double) NAN) << (any ? w[(size_t) 3 * Nmu + i] / sum_w : (double) NAN);
            for (int j = 0; j < Nt; j++) outfile << w[(size_t) 4 * Nmu + (size_t) i * Nt + j];
            outfile << endl;
        }
        outfile.close();
    });
}
