// apps/healpix_app.h -- what the two HEALPix programs share: the source's rays built, traced and classified on the device
// (kr_healpix_init_emit_dev_f64 -> kr_trace_dev_f64 -> kr_post_healpix_map_dev_f64); only the 7 npix + 6 words of the fate map come back.
#ifndef KR_HEALPIX_APP_H_
#define KR_HEALPIX_APP_H_

#include <cmath>
#include <iostream>
#include <vector>

#include "app_common.h"

namespace krapp {

struct HealpixRun {
    std::vector<double> words;       // [class | r | theta | phi | g | t | emis](npix each) + {live, disc, escape, lost, self, 0}
    int64_t npix = 0;
    kr_stats stats;
    double ms_init = 0, ms_trace = 0, ms_post = 0;

    const double* plane(int q) const { return &words[(size_t) q * (size_t) npix]; }
    double tally(int q) const { return words[7 * (size_t) npix + (size_t) q]; }
};

// `m` is completed here (npix, rays_per_pixel); redshift(-1, reverse) is the disc's Keplerian flow at the landing point
inline HealpixRun healpix_run(const kr_healpix_source& s, const kr_params& p, kr_healpix_map m, int reverse, int show_progress, bool timing)
{
    HealpixRun run;
    int64_t npix = 0;
    const int64_t n = kr_healpix_count(&s, &npix);
    if (n < 0) throw std::runtime_error(kr_last_error());
    run.npix = m.npix = npix;
    m.rays_per_pixel = s.rays_per_pixel;
    const int64_t words = 7 * npix + 6;
    Stopwatch clock;
    DeviceBuffer rays(n * (int64_t) sizeof(kr_ray_f64));
    DeviceBuffer out(words * (int64_t) sizeof(double));
    out.zero();
    check(kr_healpix_init_emit_dev_f64(&s, 0, 1, reverse, rays.get(), n, nullptr), "healpix source + redshift_start");
    if (timing) { check(kr_synchronize(nullptr), "sync"); run.ms_init = clock.lap_ms(); }
    memset(&run.stats, 0, sizeof run.stats);
    if (show_progress > 0) std::cout << "Tracing " << n << " rays of " << npix << " pixels" << std::endl;
    check(kr_trace_dev_f64(&p, rays.get(), n, nullptr, &run.stats), "trace");
    if (timing) run.ms_trace = clock.lap_ms();
    check(kr_post_healpix_map_dev_f64(p.spin, -1.0, reverse, 0, 0, -1 * M_PI, M_PI, &m, rays.get(), n, 0, 1, out.get(), nullptr), "range_phi + redshift + fate map");
    run.words.resize((size_t) words);
    check(kr_memcpy_d2h(run.words.data(), out.get(), words * (int64_t) sizeof(double)), "d2h");
    if (timing) run.ms_post = clock.lap_ms();
    return run;
}

}   // namespace krapp

#endif /* KR_HEALPIX_APP_H_ */
