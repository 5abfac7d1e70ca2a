// apps/emissivity_table.h -- the 7-column table of the reference's emissivity programs (emissivity.cpp:128-147):
// r, area, count, flux/area, emis/area, <g> = sum_g/count, <t> = sum_t/count per radial bin, TextOutput format
// (width 20, scientific, 8 digits; the count column as an integer; empty bins give nan from 0/0).  sum_z (optional: a disc with a surface) adds an
// eighth column, <z> = sum_z/count.  plunge: the comment rows "# PLUNGE" and "# R_IN" come first.
#ifndef KR_EMISSIVITY_TABLE_H_
#define KR_EMISSIVITY_TABLE_H_

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/include/text_output.h"

namespace krapp {

// raw accumulators in, table out
inline void write_emissivity_table(const std::string& out_name, int Nr, const double* bin_r, const double* bin_area, const double* count,
                                   const double* sum_flux, const double* sum_emis, const double* sum_g, const double* sum_t, const double* sum_z = nullptr, bool plunge = false,
                                   double r_in = 0)
{
    TextOutput outfile(out_name.c_str());
    if (plunge) {                          // the rows of DiscFlowKeys::write_rows (app_common.h)
        outfile << "# PLUNGE" << 1 << endl;
        outfile << "# R_IN" << r_in << endl;
    }
    for (int ir = 0; ir < Nr; ++ir) {
        const long rays = static_cast<long>(count[ir]);
        const double flux = sum_flux[ir] / bin_area[ir];
        const double emis = sum_emis[ir] / bin_area[ir];
        const double mean_g = sum_g[ir] / rays;      // 0/0 -> NaN in empty bins, as in the reference's table
        const double mean_t = sum_t[ir] / rays;
        outfile << bin_r[ir] << bin_area[ir] << rays << flux << emis << mean_g << mean_t;
        if (sum_z) outfile << sum_z[ir] / rays;
        outfile << endl;
    }
    outfile.close();
}

// reading one back (kr_line_profile, kr_disc_spectrum: emis_file): r and the emis / time columns of a 7-column emissivity table; table_r_min and the
// edge ratio from the r column, which must be log-spaced
struct EmisTable {
    std::vector<double> emis, time;
    double r_min = 0, dr = 0;
};

inline EmisTable read_emis_table(const std::string& name)
{
    std::ifstream f(name);
    if (!f) throw std::runtime_error("emis_file: cannot open " + name);
    std::vector<double> r;
    EmisTable t;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::vector<double> cols;
        std::string tok;
        while (ss >> tok) cols.push_back(strtod(tok.c_str(), nullptr));
        if (cols.empty() || line[line.find_first_not_of(" \t")] == '#') continue;          // (a table written with plunge = 1 opens with comment rows)
        if (cols.size() != 7) throw std::runtime_error("emis_file: expected 7 columns (r, area, rays, flux, emis, redshift, time) in " + name);
        r.push_back(cols[0]);
        t.emis.push_back(cols[4]);
        t.time.push_back(cols[6]);
    }
    if (r.size() < 2) throw std::runtime_error("emis_file: fewer than two radial bins in " + name);
    const size_t nr = r.size();
    t.r_min = r[0];
    t.dr = std::exp(std::log(r[nr - 1] / r[0]) / (double) (nr - 1));
    for (size_t i = 0; i < nr; ++i)
        if (!(std::fabs(r[i] / (t.r_min * std::pow(t.dr, (double) i)) - 1) <= 1e-7)) throw std::runtime_error("emis_file: the r column is not log-spaced to 1e-7 in " + name);
    return t;
}

}   // namespace krapp

#endif /* KR_EMISSIVITY_TABLE_H_ */
