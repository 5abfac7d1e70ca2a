// ref_thick_dump.cpp -- fixture generator helper (build machine only; not part of the product, never compiled by build()).
// The reference has no finite-thickness disc of its own: its RayDestination<T> is the place where a user supplies one.  This driver defines such a
// subclass -- the rules of include/kr_trace.h, KR_STOP_THICKDISC, stated here a second time, independently of host/raytracer/ray_destination.h -- and
// runs the REFERENCE's integrators to it, compiled against the reference's sources where they lie:
//     ref_thick_dump trace  <parfile>      records.txt (and init.txt with init = 1)
//     ref_thick_dump probes <parfile>      probes.txt
// trace: keys source, V, spin, dcosalpha, dbeta, cosalpha0, cosalphamax, beta0, betamax, r_max, r_out, disc_slope, disc_scale, integrator (1 RK4, 2 RK45);
// r_in = kerr_isco(spin).  PointSource -> redshift_start() -> [init.txt] -> run_raytrace(&disc, integrator, r_max) -> redshift(&disc) -> records.txt, one
// slot per line, integers in decimal, doubles as hexadecimal floats:
//     steps status rdot_sign thetadot_sign rdot_flips equatorial_crossings t r theta phi pt pr ptheta pphi redshift
// init.txt (the slots as the trace receives them):  steps rdot_sign thetadot_sign k h Q emit alpha beta
// probes: keys spin, r_out, disc_slope, disc_scale; one line per probe point,
//     r_in r_out slope scale   r theta phi prev_theta pr ptheta pphi   reached3 reached4 step_limit H rho
// with H = height(rho) whatever the range (NaN where rho is).
#include <cmath>
#include <cstdio>
#include <iostream>
#include <limits>
#include <string>
#include <vector>
using namespace std;

#include "raytracer/pointsource.h"
#include "raytracer/ray_destination.h"
#include "include/par_file.h"

// |z| <= H(rho) over r_in <= rho <= r_out (r_out <= 0: open), rho = r sin(theta), z = r cos(theta), H = slope rho + scale (1 - sqrt(r_in / rho));
// every line one IEEE operation in this association (compile with -ffp-contract=off)
class ThickDisc : public RayDestination<double> {
public:
    double r_in, r_out, slope, scale;
    ThickDisc(double r_in, double r_out, double slope, double scale) : r_in(r_in), r_out(r_out), slope(slope), scale(scale) {}

    bool in_range(double rho) const { return (rho >= r_in) && !(r_out > 0 && rho > r_out); }
    double height(double rho) const { return slope * rho + scale * (1 - sqrt(r_in / rho)); }

    bool reached(double r, double theta, double phi) const override { return reached(r, theta, phi, theta); }
    bool reached(double r, double theta, double phi, double prev) const override
    {
        const double rho = r * sin(theta), z = r * cos(theta);
        if (!in_range(rho)) return false;
        const double H = height(rho);
        return fabs(z) <= H || (prev < M_PI_2 && theta >= M_PI_2) || (prev > M_PI_2 && theta <= M_PI_2);
    }
    double step_limit(double r, double theta, double phi, double pr, double ptheta, double pphi) const override
    {
        const double big = numeric_limits<double>::max();
        const double rho = r * sin(theta), z = r * cos(theta);
        if (!in_range(rho)) return big;
        const double H = height(rho);
        const double sg = z < 0 ? -1 : 1;
        const double f = sg * z - H;
        const double zdot = pr * cos(theta) - (r * sin(theta)) * ptheta;
        const double rhodot = sin(theta) * pr + (r * cos(theta)) * ptheta;
        const double Hp = slope + (scale * 0.5 * sqrt(r_in / rho)) / rho;
        const double fdot = sg * zdot - Hp * rhodot;
        if (f > 0 && fdot < 0) {
            const double q = f / -fdot;
            return q < MIN_STEP ? MIN_STEP : q;
        }
        return big;
    }
    double velocity(double r, double theta, double phi) const override { return -1; }
    // the circular orbit at the cylindrical radius, V = 1 / (a + rho sqrt(rho)), in the association of Raytracer::ray_redshift(V = -1, projradius)
    void four_velocity(double r, double theta, double phi, double a, double et[4]) const override
    {
        const double rhosq = r * r + (a * cos(theta)) * (a * cos(theta));
        const double delta = r * r - 2 * r + a * a;
        const double sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * sin(theta) * sin(theta);
        const double e2nu = rhosq * delta / sigmasq;
        const double e2psi = sigmasq * sin(theta) * sin(theta) / rhosq;
        const double omega = 2 * a * r / sigmasq;
        const double V = 1 / (a + r * sin(theta) * sqrt(r * sin(theta)));
        et[0] = (1 / sqrt(e2nu)) / sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
        et[1] = 0;
        et[2] = 0;
        et[3] = (1 / sqrt(e2nu)) * V / sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu);
    }
};

static int run_trace(ParameterFile& par)
{
    double source[4];
    par.get_parameter_array("source", source, 4);
    const double V = par.get_parameter<double>("V", 0);
    const double spin = par.get_parameter<double>("spin");
    const double cosalpha0 = par.get_parameter<double>("cosalpha0", -0.995), cosalphamax = par.get_parameter<double>("cosalphamax", 0.995);
    const double dcosalpha = par.get_parameter<double>("dcosalpha");
    const double beta0 = par.get_parameter<double>("beta0", -1 * M_PI), betamax = par.get_parameter<double>("betamax", M_PI);
    const double dbeta = par.get_parameter<double>("dbeta");
    const double r_max = par.get_parameter<double>("r_max", 1000);
    const double r_out = par.get_parameter<double>("r_out", -1);
    const double slope = par.get_parameter<double>("disc_slope", 0), scale = par.get_parameter<double>("disc_scale", 0);
    const int integrator = par.get_parameter<int>("integrator", 1);

    PointSource<double> src(source, V, spin, TOL, dcosalpha, dbeta, cosalpha0, cosalphamax, beta0, betamax);
    src.redshift_start();
    if (par.get_parameter<int>("init", 0)) {
        FILE* f = fopen("init.txt", "w");
        for (int i = 0; i < src.get_count(); i++) {
            const Ray<double>& q = src.rays[i];
            fprintf(f, "%d %d %d %a %a %a %a %a %a\n", q.steps, q.rdot_sign, q.thetadot_sign, q.k, q.h, q.Q, q.emit, q.alpha, q.beta);
        }
        fclose(f);
    }
    ThickDisc disc(kerr_isco<double>(spin, +1), r_out, slope, scale);
    src.run_raytrace(&disc, integrator == 2 ? Integrator::RK45 : Integrator::RK4, r_max, 0);
    src.redshift(&disc);
    FILE* f = fopen("records.txt", "w");
    for (int i = 0; i < src.get_count(); i++) {
        const Ray<double>& q = src.rays[i];
        fprintf(f, "%d %d %d %d %d %d %a %a %a %a %a %a %a %a %a\n", q.steps, q.status, q.rdot_sign, q.thetadot_sign, q.rdot_flips, q.equatorial_crossings,
                q.t, q.r, q.theta, q.phi, q.pt, q.pr, q.ptheta, q.pphi, q.redshift);
    }
    fclose(f);
    return 0;
}

struct Probe { double r, theta, phi, prev, pr, ptheta, pphi; };

static int run_probes(ParameterFile& par)
{
    const double spin = par.get_parameter<double>("spin");
    const double r_out = par.get_parameter<double>("r_out", -1);
    const double slope = par.get_parameter<double>("disc_slope", 0), scale = par.get_parameter<double>("disc_scale", 0);
    const ThickDisc d(kerr_isco<double>(spin, +1), r_out, slope, scale);
    const double nan = numeric_limits<double>::quiet_NaN(), inf = numeric_limits<double>::infinity();
    vector<Probe> pts;
    unsigned long long seed = 0x9E3779B97F4A7C15ull;
    auto uni = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double) (seed >> 11) / 9007199254740992.0; };
    auto add = [&](double r, double theta, double prev, double pr, double ptheta) { pts.push_back({r, theta, 0.25, prev, pr, ptheta, 0.01}); };

    // (a) rho exactly r_in (sin(M_PI_2) is exactly 1), its neighbours, and the equator clause from either side
    for (double r : {d.r_in, nextafter(d.r_in, 0.0), nextafter(d.r_in, inf)})
        for (double prev : {M_PI_2 - 0.01, M_PI_2 + 0.01, M_PI_2}) add(r, M_PI_2, prev, -0.3, 0.02);
    // (b) z = +-H to the ulp: for fixed r the neighbouring pair of theta between which |z| <= H changes, above and below the plane
    for (int i = 0; i < 12; i++) {
        const double r = d.r_in * 1.02 * pow(r_out > 0 ? 0.97 * r_out / (d.r_in * 1.02) : 80.0, i / 11.0);
        for (int side = 0; side < 2; side++) {
            double in = M_PI_2, out = side ? M_PI_2 + 1.0 : M_PI_2 - 1.0;      // `in` satisfies |z| <= H, `out` does not
            auto inside = [&](double th) { const double rho = r * sin(th), z = r * cos(th); return fabs(z) <= d.height(rho); };
            if (!inside(in) || inside(out)) continue;
            while (true) {
                const double mid = 0.5 * (in + out);
                if (mid == in || mid == out) break;
                (inside(mid) ? in : out) = mid;
            }
            add(r, in, in, -0.5, side ? -0.03 : 0.03);
            add(r, out, out, -0.5, side ? -0.03 : 0.03);
            add(r, out, out, 0.5, side ? 0.03 : -0.03);           // moving away: no limit
        }
    }
    // (c) just outside both walls, inside the body's height
    for (double th : {M_PI_2 - 0.02, M_PI_2 + 0.02, M_PI_2 - 1e-4, 1.2, 2.0}) {
        add(nextafter(d.r_in / sin(th), 0.0) * (1 - 1e-12), th, th - 0.01, 0.2, 0.01);
        add(d.r_in / sin(th) * (1 + 1e-12), th, th - 0.01, 0.2, 0.01);
        if (r_out > 0) {
            add(r_out / sin(th) * (1 + 1e-12), th, th + 0.01, -0.2, -0.01);
            add(r_out / sin(th) * (1 - 1e-12), th, th + 0.01, -0.2, -0.01);
        }
    }
    // (d) NaN and infinite inputs
    add(nan, 1.5, 1.4, -0.1, 0.1); add(10.0, nan, 1.4, -0.1, 0.1); add(10.0, 1.5, nan, -0.1, 0.1); add(10.0, 1.5, 1.4, nan, 0.1); add(10.0, 1.5, 1.4, -0.1, nan);
    add(inf, 1.5, 1.4, -0.1, 0.1); add(10.0, 1.6, nan, -0.1, 0.1); add(10.0, 1.5, 1.4, inf, 0.1); add(0.0, 1.5, 1.4, -0.1, 0.1);
    // (f) the body stepped over: the point beyond the far face, the step before it on the other side of the plane (the equator clause alone stops
    //     the ray), on the same side (nothing does), and the same outside the radial range
    for (double r : {0.5 * d.r_in, 1.5 * d.r_in, 20.0, 300.0, 450.0})
        for (double off : {0.3, -0.3}) {
            add(r, M_PI_2 + off, M_PI_2 - off, -0.4, off > 0 ? 0.05 : -0.05);
            add(r, M_PI_2 + off, M_PI_2 + 0.5 * off, -0.4, off > 0 ? 0.05 : -0.05);
        }
    // (e) scattered points: half of them within a few heights of the surface, approaching or leaving, crossing the plane or not
    for (int i = 0; i < 120; i++) {
        const double r = exp(log(1.5) + uni() * (log(600.0) - log(1.5)));
        double theta = uni() * M_PI;
        if (i % 2) {
            const double rho = r, H = d.height(rho);
            theta = M_PI_2 + (uni() < 0.5 ? -1 : 1) * atan((H > 0 ? H : 0.01) / rho) * (0.5 + uni());
        }
        const double prev = theta + (uni() - 0.5) * 0.2;
        add(r, theta, prev, (uni() - 0.5) * 2, (uni() - 0.5) * 0.2);
    }

    FILE* f = fopen("probes.txt", "w");
    for (const Probe& p : pts) {
        const double rho = p.r * sin(p.theta);
        fprintf(f, "%a %a %a %a %a %a %a %a %a %a %a %d %d %a %a %a\n", d.r_in, d.r_out, d.slope, d.scale, p.r, p.theta, p.phi, p.prev, p.pr, p.ptheta, p.pphi,
                (int) d.reached(p.r, p.theta, p.phi), (int) d.reached(p.r, p.theta, p.phi, p.prev), d.step_limit(p.r, p.theta, p.phi, p.pr, p.ptheta, p.pphi),
                d.height(rho), rho);
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) { cerr << "usage: ref_thick_dump trace|probes <parfile>" << endl; return 2; }
    ParameterFile par(argv[2]);
    const string mode = argv[1];
    if (mode == "trace") return run_trace(par);
    if (mode == "probes") return run_probes(par);
    cerr << "unknown mode " << mode << endl;
    return 2;
}
