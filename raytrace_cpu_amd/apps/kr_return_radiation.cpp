// apps/kr_return_radiation.cpp -- the reference's disc -> disc returning-radiation program (src/return_radiation/disc_source_photonfrac_r.cpp)
// with the whole sweep over source radii resident on the MI355X, plus what that program computes and never writes: the landing map.  For every
// source radius the rays of a PointSource on the disc are generated, traced and, in one pass, wrapped in phi, redshifted (its redshift(-1), :94),
// classified and binned by landing radius (kr_post_return_map_batch_dev_f64); only the (5 Nr + 6)-word results come back, no host ray array exists.
//
// Reads (disc_source_photonfrac_r.cpp:37-59): --parfile (default ../par/disc_source_photonfrac_r.par), --outfile | outfile, source_phi = 1.5707,
// --spin | spin, cosalpha0 = -0.995, cosalphamax = 0.995, dcosalpha, dbeta (beta runs over [0, pi), :89), r_esc = 1000, --rmin | rmin = -1 (-> ISCO),
// --Nr | Nr, logbin_r = false, r_disc := the r_esc key with default 500 (sic, :56), plane_iso = true, limb = false, weight_norm = true.
// Extensions: --integrator | integrator = euler (the reference hard-codes Euler, :92), --arithmetic | KRTRACE_ARITHMETIC = hybrid|strict|fast,
// --device = 0, --timing, gamma = 2 (the EMIS plane's exponent), map_outfile (no landing map file without it).
//
// outfile: that program's table, `source_r  esc_frac  return_frac  lost_frac`, one row per radius (:128-132); the source radii are the lower edges
// of the Nr landing bins, r_min dr^ir or r_min + ir dr.  That program is stale in the reference (it calls accessors that no longer exist), so the
// classification follows its loop body and is not pinned to a build of it.
// map_outfile: a FITS file of five Nr x Nr images [i_src * Nr + j_land]: COUNT, FRACTION = weight / ray_count, ENSHIFT = flux / weight (weighted
// mean of 1 / g), EMIS = emis / ray_count, DELAY = time / weight (weighted mean arrival time); empty bins are 0 / 0 = NaN.
#include <algorithm>
#include <cmath>
#include <iostream>
#include <string>
#include <vector>
using namespace std;

#include "../host/include/fits_output.h"
#include "../host/include/kerr.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "../host/include/text_output.h"
#include "app_common.h"

int main(int argc, char** argv)
try {
    (void) kr_configure_process();       // first HIP user of this process: hardware queues for overlapping launches (include/kr_trace.h)
    const krapp::Options opt(argc, argv, "../par/disc_source_photonfrac_r.par");
    const ParameterArgs& args = opt.args;
    const ParameterFile& par = opt.par;

    const string out_name = opt.str("outfile");
    const double source_phi = par.get_parameter<double>("source_phi", 1.5707);
    const double spin = opt.req("spin");
    const double cosalpha0 = par.get_parameter<double>("cosalpha0", -0.995);
    const double cosalphamax = par.get_parameter<double>("cosalphamax", 0.995);
    const double dcosalpha = par.get_parameter<double>("dcosalpha");
    const double dbeta = par.get_parameter<double>("dbeta");
    const double r_esc = par.get_parameter<double>("r_esc", 1000);
    double r_min = opt.num("rmin", -1);
    const int Nr = opt.integer("Nr");
    const bool logbin_r = par.get_parameter<bool>("logbin_r", false);
    const double r_disc = par.get_parameter<double>("r_esc", 500);
    const bool plane_iso = par.get_parameter<bool>("plane_iso", true);
    const bool limb = par.get_parameter<bool>("limb", false);
    const bool weight_norm = par.get_parameter<bool>("weight_norm", true);
    const double gamma = par.get_parameter<double>("gamma", 2);
    const string map_name = par.get_parameter<string>("map_outfile", "");
    const string integ = opt.str("integrator", "euler");
    const string arith = krapp::arithmetic_choice(opt);
    const bool timing = opt.on_command_line("timing");
    if (Nr <= 0) throw runtime_error("Nr must be positive");

    const double r_isco = kerr_isco<double>(spin, +1);
    if (r_min == -1) r_min = r_isco;
    const double dr = logbin_r ? exp(log(r_disc / r_min) / Nr) : (r_disc - r_min) / Nr;

    // ---- one source, one landing map per radius (:66-89) --------------------------------------------------------------------------
    vector<kr_pointsource> src(static_cast<size_t>(Nr));
    vector<kr_return_map> maps(static_cast<size_t>(Nr));
    vector<int64_t> count(static_cast<size_t>(Nr));
    vector<double> source_r(static_cast<size_t>(Nr));
    int64_t n_max = 0;
    for (int ir = 0; ir < Nr; ++ir) {
        source_r[ir] = logbin_r ? r_min * pow(dr, ir) : r_min + ir * dr;
        kr_pointsource& s = src[ir];
        memset(&s, 0, sizeof s);
        s.pos[0] = 0; s.pos[1] = source_r[ir]; s.pos[2] = M_PI_2 - 1E-6; s.pos[3] = source_phi;
        s.V = disc_velocity<double>(source_r[ir], spin, +1);
        s.spin = spin; s.tol = 100; s.E = 1;
        s.cosalpha0 = cosalpha0; s.cosalphamax = cosalphamax; s.dcosalpha = dcosalpha;
        s.beta0 = 0; s.betamax = M_PI; s.dbeta = dbeta;
        count[ir] = kr_pointsource_count(&s, nullptr, nullptr);
        if (count[ir] <= 0) throw runtime_error("empty ray grid");
        n_max = max(n_max, count[ir]);
        kr_return_map& m = maps[ir];
        memset(&m, 0, sizeof m);
        m.cls.r_isco = r_isco; m.cls.r_disc = r_disc; m.cls.r_esc = r_esc; m.cls.source_r = source_r[ir]; m.cls.source_phi = source_phi;
        m.cls.plane_iso = plane_iso; m.cls.limb = limb; m.cls.weight_norm = weight_norm;
        m.r_min = r_min; m.dr = dr; m.gamma = gamma; m.nr = Nr; m.logbin = logbin_r ? 1 : 0;
    }

    kr_params p;
    kr_params_default(&p, spin);
    p.integrator = krapp::integrator_code(integ, KR_EULER);
    p.theta_max = M_PI_2;
    p.r_max = 1.1 * r_esc;
    p.stop_kind = KR_STOP_THETA;
    p.flags = krapp::arithmetic_flags(arith, p.integrator);

    // ---- device pipeline: the radii in groups whose ray buffers stay under a quarter of the device's memory ---------------------------
    krapp::require_device();             // before the output file is created
    krapp::check(kr_set_device(args.get_parameter<int>("--device", 0)), "kr_set_device");
    int64_t hbm = 0;
    krapp::check(kr_device_info(nullptr, nullptr, &hbm, nullptr, 0), "kr_device_info");
    const int64_t slot = (n_max * (int64_t) sizeof(kr_ray_f64) + 255) / 256 * 256;
    const int per_group = (int) max<int64_t>(1, min<int64_t>(min<int64_t>(256, Nr), (hbm / 4) / slot));
    const int64_t words = 5 * (int64_t) Nr + 6;
    krapp::Stopwatch wall, clock;
    krapp::DeviceBuffer rays(per_group * slot);
    krapp::DeviceBuffer out(Nr * words * (int64_t) sizeof(double));
    out.zero();
    kr_stats total;
    memset(&total, 0, sizeof total);
    double ms_init = 0, ms_trace = 0, ms_post = 0;
    for (int first = 0; first < Nr; first += per_group) {
        const int k = min(per_group, Nr - first);
        vector<void*> d_rays(static_cast<size_t>(k)), d_out(static_cast<size_t>(k)), tickets(static_cast<size_t>(k), nullptr);
        vector<const kr_params*> pp(static_cast<size_t>(k), &p);
        vector<double> V(static_cast<size_t>(k));
        for (int q = 0; q < k; ++q) {
            d_rays[q] = static_cast<char*>(rays.get()) + q * slot;
            d_out[q] = static_cast<double*>(out.get()) + (first + q) * words;
            V[q] = src[first + q].V;
        }
        krapp::check(kr_pointsource_init_emit_batch_dev_f64(k, &src[first], V.data(), 0, 0, d_rays.data(), &count[first], nullptr), "pointsource_init + redshift_start");
        if (timing) { krapp::check(kr_synchronize(nullptr), "sync"); ms_init += clock.lap_ms(); }
        krapp::check(kr_trace_batch_async_f64(k, pp.data(), d_rays.data(), &count[first], nullptr, tickets.data()), "trace");
        const int rc_post = kr_post_return_map_batch_dev_f64(k, spin, -1.0, 0, 0, 0, -1 * M_PI, M_PI, &maps[first], d_rays.data(), &count[first], d_out.data(), nullptr);
        const string post_error = rc_post == KR_OK ? string() : string(kr_last_error());
        kr_stats st;
        krapp::check(kr_trace_wait_many(k, tickets.data(), nullptr, &st), "trace");       // retires the tickets whatever the pass said
        if (rc_post != KR_OK) throw runtime_error("range_phi + redshift + landing map: " + post_error);
        if (timing) ms_trace += clock.lap_ms();
        krapp::check(kr_synchronize(nullptr), "sync");                                    // the buffers are reused by the next group
        if (timing) ms_post += clock.lap_ms();
        total.rays_traced += st.rays_traced; total.steps_total += st.steps_total; total.kernel_ms += st.kernel_ms;
    }
    vector<double> h(static_cast<size_t>(Nr * words));
    krapp::check(kr_memcpy_d2h(h.data(), out.get(), (int64_t) (h.size() * sizeof(double))), "d2h");
    const double ms_device = wall.lap_ms();

    // ---- the table of :128-132 -----------------------------------------------------------------------------------------------------
    {
        TextOutput outfile(out_name.c_str());
        for (int ir = 0; ir < Nr; ++ir) {
            const double* s = &h[ir * words + 5 * (int64_t) Nr];                          // ray_count, return, escape, lost
            const double esc_frac = s[2] / s[0], return_frac = s[1] / s[0], lost_frac = s[3] / s[0];
            outfile << source_r[ir] << esc_frac << return_frac << lost_frac << endl;
        }
        outfile.close();
    }

    // ---- the landing map ------------------------------------------------------------------------------------------------------------
    if (!map_name.empty()) {
        const size_t npix = (size_t) Nr * Nr;
        vector<vector<double>> img(5, vector<double>(npix));
        for (int i = 0; i < Nr; ++i) {
            const double* w = &h[i * words];
            const double ray_count = w[5 * (int64_t) Nr];
            for (int j = 0; j < Nr; ++j) {
                const double cnt = w[j], weight = w[Nr + j], flux = w[2 * (int64_t) Nr + j], emis = w[3 * (int64_t) Nr + j], time = w[4 * (int64_t) Nr + j];
                const size_t px = (size_t) i * Nr + j;
                img[0][px] = cnt;
                img[1][px] = cnt > 0 ? weight / ray_count : NAN;                          // an empty bin is NaN in every derived plane, as in the image program
                img[2][px] = flux / weight;
                img[3][px] = cnt > 0 ? emis / ray_count : NAN;
                img[4][px] = time / weight;
            }
        }
        FITSOutput<double> fits(map_name);
        fits.create_primary();
        fits.write_comment("Kerr BH returning radiation: landing map per source radius");
        fits.write_keyword("GENERATOR", "Simulation results were generated by this software", "kr_return_radiation");
        fits.write_keyword("SPIN", "Black hole spin parameter a/M", spin);
        fits.write_keyword("RMIN", "First edge of the radial bins (rg)", r_min);
        fits.write_keyword("DR", "Bin width (rg), or ratio between edges with LOGBIN", dr);
        fits.write_keyword("LOGBIN", "1 = logarithmic radial bins", logbin_r ? 1 : 0);
        fits.write_keyword("NR", "Number of source radii and of landing bins", Nr);
        fits.write_keyword("GAMMA", "EMIS sums weight / g^GAMMA", gamma);
        fits.write_keyword("PLANEISO", "1 = rays weighted by |sin(alpha) sin(beta)|", plane_iso ? 1 : 0);
        fits.write_keyword("LIMB", "1 = limb darkening 1 + 2.06 |sin(alpha) sin(beta)|", limb ? 1 : 0);
        fits.write_keyword("WGTNORM", "1 = fractions normalised by the summed weight", weight_norm ? 1 : 0);
        const char* names[5] = {"COUNT", "FRACTION", "ENSHIFT", "EMIS", "DELAY"};
        const char* what[5] = {"Rays of source radius i binned at landing radius j", "Weight landing in bin j over the source's ray_count",
                               "Weighted mean of emitted / received energy, 1 / g", "Sum of weight / g^GAMMA over the source's ray_count",
                               "Weighted mean coordinate time of arrival"};
        for (int k = 0; k < 5; ++k) {
            vector<double*> rows(static_cast<size_t>(Nr));
            for (int i = 0; i < Nr; ++i) rows[i] = &img[k][(size_t) i * Nr];
            fits.write_image(rows.data(), Nr, Nr, false);
            fits.set_ext_name(names[k]);
            fits.write_comment(what[k]);
            fits.write_comment("[i_src * NR + j_land]; empty bins are NaN");
        }
        fits.close();
    }

    if (timing)
        cout << "timing: radii " << Nr << " in groups of " << per_group << " rays " << total.rays_traced << " steps " << total.steps_total << " | init+redshift_start "
             << ms_init << " ms | trace " << ms_trace << " ms (kernels " << total.kernel_ms << ") | range_phi+redshift+landing map " << ms_post << " ms | device total "
             << ms_device << " ms | files " << wall.lap_ms() << " ms" << endl;
    cout << "Done" << endl;
    return 0;
} catch (const exception& e) {
    cerr << e.what() << endl;
    return 1;
}
