// ref_paths_dump.cpp -- fixture generator helper (build machine only; not part of the product, never compiled by build()).
// The reference's two ray-path programs hard-wire Integrator::Euler, so the RK4 write paths of Raytracer<T>::run_raytrace -- the theta-limit
// overload and the RayDestination overload -- are reached through this small driver, compiled AGAINST the reference's sources where they lie:
//     ref_paths_dump <parfile>
// Parameter file: the keys of trace_rays (outfile, source, V, spin, cosalpha0, cosalphamax, dcosalpha, beta0, betamax, dbeta, r_max, theta_max,
// write_step, write_rmin, write_rmax, write_cartesian) plus  dest = 0 | 1  (1: DiscWithISCODestination(kerr_isco(spin), r_out)), r_out = -1 and
// records = 0 | 1  (1: the final record of every ray goes to records.txt -- integers in decimal, doubles as hexadecimal floats, one ray per line:
// steps status rdot_sign thetadot_sign rdot_flips equatorial_crossings t r theta phi pt pr ptheta pphi).
#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
using namespace std;

#include "raytracer/pointsource.h"
#include "raytracer/ray_destination.h"
#include "include/par_file.h"

int main(int argc, char** argv)
{
    if (argc != 2) { cerr << "usage: ref_paths_dump <parfile>" << endl; return 2; }
    ParameterFile par(argv[1]);
    const string out_name = par.get_parameter<string>("outfile");
    double source[4];
    par.get_parameter_array("source", source, 4);
    const double V = par.get_parameter<double>("V", 0);
    const double spin = par.get_parameter<double>("spin");
    const double cosalpha0 = par.get_parameter<double>("cosalpha0", -0.995), cosalphamax = par.get_parameter<double>("cosalphamax", 0.995);
    const double dcosalpha = par.get_parameter<double>("dcosalpha");
    const double beta0 = par.get_parameter<double>("beta0", -1 * M_PI), betamax = par.get_parameter<double>("betamax", M_PI);
    const double dbeta = par.get_parameter<double>("dbeta");
    const double r_max = par.get_parameter<double>("r_max", 100);
    const double theta_max = par.get_parameter<double>("theta_max", M_PI_2);
    const int write_step = (int) par.get_parameter<double>("write_step", 10);
    const double write_rmin = par.get_parameter<double>("write_rmin", -1), write_rmax = par.get_parameter<double>("write_rmax", -1);
    const bool write_cartesian = par.get_parameter<double>("write_cartesian", true);
    const int dest = par.get_parameter<int>("dest", 0);
    const double r_out = par.get_parameter<double>("r_out", -1);

    TextOutput outfile(out_name);
    PointSource<double> src(source, V, spin, TOL, dcosalpha, dbeta, cosalpha0, cosalphamax, beta0, betamax);
    if (dest == 0) {
        src.run_raytrace(Integrator::RK4, theta_max, r_max, 0, &outfile, write_step, write_rmax, write_rmin, write_cartesian);
    } else {
        DiscWithISCODestination<double> disc(kerr_isco<double>(spin, +1), r_out);
        src.run_raytrace(&disc, Integrator::RK4, r_max, 0, &outfile, write_step, write_rmax, write_rmin, write_cartesian);
    }
    outfile.close();
    if (par.get_parameter<int>("records", 0)) {
        FILE* f = fopen("records.txt", "w");
        for (int i = 0; i < src.get_count(); i++) {
            const Ray<double>& q = src.rays[i];
            fprintf(f, "%d %d %d %d %d %d %a %a %a %a %a %a %a %a\n", q.steps, q.status, q.rdot_sign, q.thetadot_sign, q.rdot_flips, q.equatorial_crossings,
                    q.t, q.r, q.theta, q.phi, q.pt, q.pr, q.ptheta, q.pphi);
        }
        fclose(f);
    }
    return 0;
}
