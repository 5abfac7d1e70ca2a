// apps/volume_app.h -- what kr_volume_map and kr_volume_spectrum share: the mapper's grid and the source trace as the parameter file names them, the
// point source, the proper volume of a cell and the FITS keywords both files carry.
#ifndef KR_APP_VOLUME_APP_H_
#define KR_APP_VOLUME_APP_H_

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../host/include/fits_output.h"
#include "../host/include/par_args.h"
#include "../host/include/par_file.h"
#include "app_common.h"

namespace krapp {

// r0 (first radial edge), rmax, Nr, Ntheta, Nphi = 1, logbin_r = false, theta_max = pi / 2 and r_esc = 1000 (where the source trace stops), mode = 0,
// --integrator | integrator = rk4
struct VolumeGridPar {
    double r0, rmax, theta_max, r_esc;
    int Nr, Ntheta, Nphi, mode;
    bool logbin_r;
    std::string integ;

    VolumeGridPar(ParameterArgs& args, ParameterFile& par)
    {
        r0 = par.get_parameter<double>("r0");
        rmax = par.get_parameter<double>("rmax");
        Nr = par.get_parameter<int>("Nr");
        Ntheta = par.get_parameter<int>("Ntheta");
        Nphi = par.get_parameter<int>("Nphi", 1);
        logbin_r = par.get_parameter<bool>("logbin_r", false);
        theta_max = par.get_parameter<double>("theta_max", M_PI_2);
        r_esc = par.get_parameter<double>("r_esc", 1000);
        mode = par.get_parameter<int>("mode", 0);
        integ = args.key_exists("--integrator") ? args.get_parameter<std::string>("--integrator") : par.get_parameter<std::string>("integrator", "rk4");
        if (Nr < 1 || Ntheta < 1 || Nphi < 1) throw std::runtime_error("Nr, Ntheta and Nphi must be at least 1");
    }

    // The grid has the bin widths of Mapper's constructor (mapper.cpp:14-16: n - 1 divisions of [r0, rmax], [0, pi / 2], [0, 2 pi]; an axis of one cell
    // spans the whole range); the energy shift is measured by the mapper's observers, on orbits of V = 1 / (a + r sin(theta) sqrt(r sin(theta))).
    kr_volume_map map() const
    {
        kr_volume_map m;
        memset(&m, 0, sizeof m);
        m.r_min = r0;
        m.dr = logbin_r ? exp(log(rmax / r0) / std::max(Nr - 1, 1)) : (rmax - r0) / std::max(Nr - 1, 1);
        m.dtheta = (M_PI_2) / std::max(Ntheta - 1, 1);
        m.dphi = (2 * M_PI) / std::max(Nphi - 1, 1);
        m.V = -1; m.projradius = 1; m.reverse = 0; m.motion = 0;
        m.nr = Nr; m.ntheta = Ntheta; m.nphi = Nphi; m.logbin = logbin_r ? 1 : 0; m.mode = mode;
        return m;
    }

    // the trace of the source's rays
    kr_params params(double spin) const
    {
        kr_params p;
        kr_params_default(&p, spin);
        p.integrator = integrator_code(integ, KR_RK4);
        p.theta_max = theta_max;
        p.r_max = r_esc;
        p.stop_kind = KR_STOP_THETA;
        p.flags = 0;                         // the map rides the strict recording loop
        return p;
    }
};

// source[4], cosalpha0 = -0.995, cosalphamax = 0.995, dcosalpha, beta0 = -pi, betamax = pi, dbeta
inline kr_pointsource read_point_source(ParameterFile& par, double spin, double V)
{
    kr_pointsource src;
    memset(&src, 0, sizeof src);
    par.get_parameter_array("source", src.pos, 4);
    src.V = V; src.spin = spin; src.tol = 100; src.E = 1;
    src.cosalpha0 = par.get_parameter<double>("cosalpha0", -0.995);
    src.cosalphamax = par.get_parameter<double>("cosalphamax", 0.995);
    src.dcosalpha = par.get_parameter<double>("dcosalpha");
    src.beta0 = par.get_parameter<double>("beta0", -1 * M_PI);
    src.betamax = par.get_parameter<double>("betamax", M_PI);
    src.dbeta = par.get_parameter<double>("dbeta");
    return src;
}

// calculate_volume (mapper.cpp:311-338): sqrt(-g_rr g_thth g_phph) dr dtheta dphi at the lower corner of the cells (ir, itheta, *)
inline double cell_volume(const kr_volume_map& m, double spin, int ir, int itheta)
{
    const double a = spin;
    const double r = m.logbin ? m.r_min * pow(m.dr, ir) : m.r_min + m.dr * ir;
    const double this_bin_dr = m.logbin ? r * (m.dr - 1) : m.dr;
    const double theta = itheta * m.dtheta;
    const double rhosq = r * r + (a * cos(theta)) * (a * cos(theta));
    const double delta = r * r - 2 * r + a * a;
    const double sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * sin(theta) * sin(theta);
    const double e2psi = sigmasq * sin(theta) * sin(theta) / rhosq;
    const double grr = -rhosq / delta, gthth = -rhosq, gphph = -e2psi;
    return sqrt(-1 * grr * gthth * gphph) * this_bin_dr * m.dtheta * m.dphi;
}

// the radial-axis keywords of both files
inline void write_grid_keywords(FITSOutput<double>& fits, const VolumeGridPar& g, const kr_volume_map& m)
{
    fits.write_keyword("R0", "First radial edge (rg)", g.r0);
    fits.write_keyword("RMAX", "Lower edge of the last radial cell (rg)", g.rmax);
    fits.write_keyword("NR", "Radial cells", g.Nr);
    fits.write_keyword("DR", "Cell width (rg), or ratio between edges with LOGBIN_R", m.dr);
    fits.write_keyword("LOGBIN_R", "1 = logarithmic radial cells", g.logbin_r ? 1 : 0);
}

}   // namespace krapp

#endif /* KR_APP_VOLUME_APP_H_ */
