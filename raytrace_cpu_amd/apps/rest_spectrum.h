// apps/rest_spectrum.h -- the tabulated rest-frame spectrum of the programs that smear one over the disc (kr_disc_spectrum, kr_reverb_response): the
// two-column reader, the resampler onto the log grid of a kr_spectrum_model, and the keys spec_file, Nzones and spec_bins.
//   spec_file       two-column text, energy and value per line, energies ascending (the format of the reference's spectrum reader); a
//                   comma-separated list (no blanks) gives one file per radial zone, innermost first (zones log-spaced over [r_isco, r_disc))
//   Nzones          optional; must equal the number of files
//   spec_bins = 512 nodes of the log grid the files are resampled onto (linear in log E), from the first file's first to its last energy
#ifndef KR_APP_REST_SPECTRUM_H_
#define KR_APP_REST_SPECTRUM_H_

#include <cmath>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "app_common.h"

namespace krapp {

struct TwoColumns { std::vector<double> energy, value; };

inline TwoColumns read_spectrum(const std::string& name)
{
    std::ifstream f(name);
    if (!f) throw std::runtime_error("spec_file: cannot open " + name);
    TwoColumns t;
    double e, v;
    while (f >> e >> v) { t.energy.push_back(e); t.value.push_back(v); }
    if (t.energy.size() < 2) throw std::runtime_error("spec_file: fewer than two rows in " + name);
    for (size_t i = 0; i < t.energy.size(); ++i)
        if (!(t.energy[i] > 0) || (i > 0 && !(t.energy[i] > t.energy[i - 1]))) throw std::runtime_error("spec_file: the energies must be positive and ascending in " + name);
    return t;
}

// the file's value at energy e, linear in log E between its points, the end values beyond them (api.resample_spectrum: numpy.interp)
inline double interpolate(const TwoColumns& t, double e)
{
    const size_t n = t.energy.size();
    const double le = log(e);
    if (le <= log(t.energy[0])) return t.value[0];
    if (le >= log(t.energy[n - 1])) return t.value[n - 1];
    size_t k = 0;
    while (k + 2 < n && le >= log(t.energy[k + 1])) ++k;
    const double l0 = log(t.energy[k]), l1 = log(t.energy[k + 1]);
    return t.value[k] + (le - l0) / (l1 - l0) * (t.value[k + 1] - t.value[k]);
}

inline std::vector<std::string> split_commas(const std::string& s)
{
    std::vector<std::string> out;
    std::string item;
    std::istringstream ss(s);
    while (getline(ss, item, ',')) {
        const size_t a = item.find_first_not_of(" \t"), b = item.find_last_not_of(" \t");
        if (a != std::string::npos) out.push_back(item.substr(a, b - a + 1));
    }
    return out;
}

// the files of spec_file on the log grid: S[z][k] at node first pow(s_de, k), the last node never beyond the file's last energy
struct RestSpectrum {
    std::vector<double> S;
    int nz = 0, s_ne = 0;
    double s_e_min = 0, s_de = 0;

    // model = 1 and the grid into the model; S must outlive it
    void fill(kr_spectrum_model& sm) const
    {
        sm.model = 1;
        sm.nz = (int32_t) nz;
        sm.s_ne = s_ne;
        sm.s_e_min = s_e_min;
        sm.s_de = s_de;
        sm.s = S.data();
    }
    void print() const { std::cout << "rest-frame spectrum: " << nz << " zone(s), " << s_ne << " nodes from " << s_e_min << ", ratio " << s_de << std::endl; }
};

inline RestSpectrum read_rest_spectrum(const Options& opt, const char* needs = "model = table needs spec_file")
{
    const std::vector<std::string> files = split_commas(opt.str("spec_file", ""));
    if (files.empty()) throw std::invalid_argument(needs);
    if (opt.has("Nzones") && (int) opt.num("Nzones", 1) != (int) files.size()) throw std::invalid_argument("Nzones: must equal the number of files in spec_file");
    const int spec_bins = (int) opt.num("spec_bins", 512);
    if (spec_bins < 2) throw std::invalid_argument("spec_bins: at least two nodes");
    std::vector<TwoColumns> specs;
    for (const std::string& f : files) specs.push_back(read_spectrum(f));
    const double first = specs[0].energy.front(), last = specs[0].energy.back();
    RestSpectrum r;
    r.nz = (int) files.size();
    r.s_ne = spec_bins;
    r.s_e_min = first;
    r.s_de = exp(log(last / first) / (spec_bins - 1));
    r.S.resize(files.size() * (size_t) spec_bins);
    for (size_t z = 0; z < files.size(); ++z)
        for (int k = 0; k < spec_bins; ++k) {
            double node = first * pow(r.s_de, k);
            if (k == spec_bins - 1 && node > last) node = last;
            r.S[z * (size_t) spec_bins + (size_t) k] = interpolate(specs[z], node);
        }
    return r;
}

}   // namespace krapp

#endif /* KR_APP_REST_SPECTRUM_H_ */
