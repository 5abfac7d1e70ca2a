// apps/kr_emissivity.cpp -- the reference's `emissivity` program (src/emissivity/emissivity.cpp) with the whole ray
// pipeline resident on the MI355X: rays are generated, traced, redshifted and binned in HBM; only the Nr-bin
// histogram comes back.  Same parameter file, same command-line overrides, same 7-column output table
// (r, area, count, flux/area, emis/area, <g>, <t>; TextOutput format).
//
// Reads (emissivity.cpp:17-55): --parfile (default ../par/emissivity.par), --outfile | outfile, source[4], V = 0,
// --spin | spin, cosalpha0 = -0.995, cosalphamax = 0.995, dcosalpha, beta0 = -pi, betamax = pi, dbeta, r_esc = 1000
// (outer radius of the trace), --rmin | rmin = -1 (-> ISCO), --Nr | Nr = 100, r_disc := r_esc key, default 500 (sic, :51),
// logbin_r = true, gamma = 2, --source_h.  Extensions: --integrator | integrator = rk45 (the reference hard-codes RK45,
// :91; BASELINE configs[1] is the same run with rk4), --arithmetic | KRTRACE_ARITHMETIC = hybrid|strict|fast,
// --device = 0, --timing.  --Nmu | Nmu = 0 and --mu_outfile | mu_outfile: with Nmu >= 1 the histogram is also split by the incidence angle in the
// disc frame (kr_post_emissivity_mu_dev_f64) and a second table goes to mu_outfile: per radial bin r, then Nmu columns count2 / count (the share
// of the bin's rays in each mu bin) and the mean mu, in TextOutput's format.  Without Nmu the program does what it did before the key existed.
// disc_slope, disc_scale (and disc_rin = ISCO): with either key the disc has a surface, z = +-H(rho), H = disc_slope rho + disc_scale (1 - sqrt(disc_rin / rho))
// between disc_rin and r_disc (KR_STOP_THICKDISC, include/kr_trace.h): the rays stop on it (RK4 / RK45), the gas orbits at the cylindrical radius rho,
// the histogram is over rho (kr_post_emissivity_surface_dev_f64), the areas are those of the surface's rings (integrate_surface_area, disc.h) and the
// table gets an eighth column, the mean landing height <z> of the bin.  Not with Nmu.  Without the keys the program and its output are what they were.
// plunge = 0 | 1, r_in (app_common.h, DiscFlowKeys): with plunge = 1 the gas plunges inside the ISCO (V = KR_V_PLUNGE, include/kr_trace.h), rmin
// defaults to r_in = 1.02 x the horizon radius and the table (and the mu table) opens with the rows "# PLUNGE" and "# R_IN"; the area column is
// integrate_disc_area's as ever, whose plunge branch serves the annuli below the ISCO.  Not with a thick disc.  plunge = 0: what the program did.
//
// What is NOT taken from the reference: with logbin_r = 0 its bin areas do not compile (`disc_r + dr`, :79); the
// intended upper edge r + dr (as in emissivity_rd.cpp:88 ... which passes `dr` alone) is used here.
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/disc.h"
#include "../host/include/kerr.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "app_common.h"
#include "emissivity_table.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();       // first HIP user of this process: hardware queues for overlapping launches (include/kr_trace.h)
    const krapp::Options opt(argc, argv, "../par/emissivity.par");
    const ParameterArgs& args = opt.args;
    const ParameterFile& par = opt.par;

    const string out_name = opt.str("outfile");
    double source[4];
    par.get_parameter_array("source", source, 4);
    if (args.key_exists("--source_h")) source[1] = args.get_parameter<double>("--source_h");
    const double V = par.get_parameter<double>("V", 0);
    const double spin = opt.req("spin");
    const double r_max = par.get_parameter<double>("r_esc", 1000);
    double r_min = opt.num("rmin", -1);
    const int Nr = opt.integer("Nr", 100);
    const double r_disc = par.get_parameter<double>("r_esc", 500);
    const bool logbin_r = par.get_parameter<bool>("logbin_r", true);
    const double gamma = par.get_parameter<double>("gamma", 2);
    const string integ = opt.str("integrator", "rk45");
    const string arith = krapp::arithmetic_choice(opt);
    const bool timing = opt.on_command_line("timing");
    const int Nmu = opt.integer("Nmu", 0);
    const string mu_out_name = opt.str("mu_outfile", "");
    if (Nmu < 0) throw invalid_argument("Nmu must be >= 0");
    if (Nmu > 0 && mu_out_name.empty()) throw invalid_argument("Nmu needs mu_outfile");
    const bool thick = par.key_exists("disc_slope") || par.key_exists("disc_scale");
    const double disc_slope = par.get_parameter<double>("disc_slope", 0), disc_scale = par.get_parameter<double>("disc_scale", 0);
    const krapp::DiscFlowKeys flow = krapp::disc_flow_keys(opt, spin);         // plunge = 0 | 1, r_in: the gas inside the ISCO, and the table from r_in
    if (thick && flow.plunge) throw invalid_argument("plunge: the surface of a thick disc keeps the Keplerian flow (no disc_slope / disc_scale)");
    if (thick && Nmu > 0) throw invalid_argument("disc_slope / disc_scale: the incidence angle to a tilted surface is not offered (no Nmu)");

    kr_pointsource src;
    memset(&src, 0, sizeof src);
    for (int i = 0; i < 4; ++i) src.pos[i] = source[i];
    src.V = V;
    src.spin = spin;
    src.tol = 100;   // TOL, raytracer.h
    src.E = 1;
    src.cosalpha0 = par.get_parameter<double>("cosalpha0", -0.995);
    src.cosalphamax = par.get_parameter<double>("cosalphamax", 0.995);
    src.dcosalpha = par.get_parameter<double>("dcosalpha");
    src.beta0 = par.get_parameter<double>("beta0", -1 * M_PI);
    src.betamax = par.get_parameter<double>("betamax", M_PI);
    src.dbeta = par.get_parameter<double>("dbeta");

    // radial bins and their proper areas (host: Nr x 49 small tetrad evaluations)
    const double r_isco = kerr_isco<double>(spin, +1);
    if (r_min < 0) r_min = flow.inner_edge(r_isco);
    const double disc_rin = par.get_parameter<double>("disc_rin", r_isco);
    const double dr = logbin_r ? exp(log(r_disc / r_min) / Nr) : (r_disc - r_min) / Nr;
    vector<double> bin_r(Nr), bin_area(Nr);
    for (int ir = 0; ir < Nr; ++ir) {
        bin_r[ir] = logbin_r ? r_min * pow(dr, ir) : r_min + ir * dr;
        const double bin_top = logbin_r ? bin_r[ir] * dr : bin_r[ir] + dr;
        bin_area[ir] = thick ? integrate_surface_area(bin_r[ir], bin_top, disc_rin, disc_slope, disc_scale, spin) : integrate_disc_area(bin_r[ir], bin_top, spin);
    }
    const long num_primary_rays = (((src.cosalphamax - src.cosalpha0) / src.dcosalpha) * ((src.betamax - src.beta0) / src.dbeta));

    kr_emis_bins bins;
    memset(&bins, 0, sizeof bins);
    bins.r_min = r_min;
    bins.dr = dr;
    bins.r_isco = flow.inner_edge(r_isco);
    bins.gamma = gamma;
    bins.spin = spin;
    bins.num_primary_rays = static_cast<double>(num_primary_rays);
    bins.nr = Nr;
    bins.logbin = logbin_r ? 1 : 0;

    kr_params p;
    kr_params_default(&p, spin);
    p.integrator = krapp::integrator_code(integ, KR_RK45);
    p.theta_max = M_PI_2;
    p.r_max = r_max;
    p.stop_kind = KR_STOP_THETA;
    p.flags = krapp::arithmetic_flags(arith, p.integrator);
    if (thick) {
        p.stop_kind = KR_STOP_THICKDISC;
        p.stop_params[0] = disc_rin; p.stop_params[1] = r_disc; p.stop_params[2] = disc_slope; p.stop_params[3] = disc_scale;
    }

    // ---- device pipeline ------------------------------------------------------------------------------------------
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    krapp::Stopwatch clock;
    const int64_t n = kr_pointsource_count(&src, nullptr, nullptr);
    if (n <= 0) throw runtime_error("empty ray grid");
    krapp::DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    krapp::DeviceBuffer hist((6 * (int64_t) Nr + 4) * (int64_t) sizeof(double));      // (the surface form's six planes and four tallies; the flat form uses 5 Nr + 1)
    hist.zero();
    krapp::check(kr_pointsource_init_emit_dev_f64(&src, 0, 1, V, 0, 0, rays.get(), n, nullptr), "pointsource_init + redshift_start");
    krapp::check(kr_synchronize(nullptr), "sync");
    const double ms_init = clock.lap_ms();
    kr_stats st;
    krapp::check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &st), "trace");
    const double ms_trace = clock.lap_ms();
    vector<double> hmu;
    if (Nmu > 0) {
        kr_mu_bins mb;
        memset(&mb, 0, sizeof mb);
        mb.nmu = Nmu;
        hmu.resize((2 * (size_t) Nmu + 1) * (size_t) Nr + 3);
        krapp::DeviceBuffer by_mu((int64_t) (hmu.size() * sizeof(double)));
        by_mu.zero();
        krapp::check(kr_post_emissivity_mu_dev_f64(spin, flow.V(), 0, 0, 0, -1 * M_PI, M_PI, &bins, &mb, rays.get(), n, hist.get(), by_mu.get(), nullptr),
                     "range_phi + redshift + histogram by angle");
        krapp::check(kr_memcpy_d2h(hmu.data(), by_mu.get(), (int64_t) (hmu.size() * sizeof(double))), "d2h");
    } else if (thick) {
        krapp::check(kr_post_emissivity_surface_dev_f64(spin, 0, -1 * M_PI, M_PI, &bins, rays.get(), n, hist.get(), nullptr), "range_phi + redshift + surface histogram");
    } else {
        krapp::check(kr_post_emissivity_dev_f64(spin, flow.V(), 0, 0, 0, -1 * M_PI, M_PI, &bins, rays.get(), n, hist.get(), nullptr), "range_phi + redshift + histogram");
    }
    vector<double> h(thick ? 6 * (size_t) Nr + 4 : 5 * (size_t) Nr + 1);
    krapp::check(kr_memcpy_d2h(h.data(), hist.get(), (int64_t) (h.size() * sizeof(double))), "d2h");
    const double ms_post = clock.lap_ms();

    // ---- the divisions of emissivity.cpp:128-134 and the table ---------------------------------------------------------
    krapp::write_emissivity_table(out_name, Nr, bin_r.data(), bin_area.data(), &h[0], &h[Nr], &h[2 * (size_t) Nr], &h[3 * (size_t) Nr], &h[4 * (size_t) Nr],
                                  thick ? &h[5 * (size_t) Nr] : nullptr, flow.plunge, flow.r_in);

    if (Nmu > 0) {
        // count2 / count per mu bin (count: the radial histogram's, so a bin's bad-angle rays are missing from its row) and the mean mu over the
        // rays that have an angle (the row sum of count2); 0/0 -> NaN in empty bins
        const size_t plane = (size_t) Nr * Nmu;
        TextOutput mu_out(mu_out_name.c_str());
        flow.write_rows(mu_out);
        for (int ir = 0; ir < Nr; ++ir) {
            double row = 0;
            for (int im = 0; im < Nmu; ++im) row += hmu[(size_t) ir * Nmu + im];
            mu_out << bin_r[ir];
            for (int im = 0; im < Nmu; ++im) mu_out << hmu[(size_t) ir * Nmu + im] / h[ir];
            mu_out << hmu[2 * plane + ir] / row << endl;
        }
        mu_out.close();
        cout << static_cast<long>(hmu[hmu.size() - 1]) << " of " << static_cast<long>(hmu[hmu.size() - 2]) << " binned rays have no incidence angle (bad-angle)" << endl;
    }

    if (timing)
        cout << "timing: rays " << st.rays_traced << " steps " << st.steps_total << " | init+redshift_start " << ms_init << " ms | trace " << ms_trace
             << " ms (kernel " << st.kernel_ms << ") | range_phi+redshift+histogram+readback " << ms_post << " ms | disc rays " << static_cast<long>(h[(thick ? 6 : 5) * (size_t) Nr]) << endl;
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
