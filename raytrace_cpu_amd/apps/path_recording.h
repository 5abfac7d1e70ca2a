// apps/path_recording.h -- what kr_trace_rays and kr_trace_rays_imageplane share: the rays are on the device already; their paths are counted,
// recorded, read back once and written as the reference's trajectory file (run_raytrace's serial branch, raytracer.cpp:86-100: one row per
// line through TextOutput, two blank lines after every traced ray).
#ifndef KR_APP_PATH_RECORDING_H_
#define KR_APP_PATH_RECORDING_H_

#include <iostream>
#include <string>
#include <vector>

#include "../host/include/kerr.h"
#include "../host/include/text_output.h"
#include "app_common.h"

namespace krapp {

struct PathTimes {
    double count_ms = 0, record_ms = 0, readback_ms = 0, text_ms = 0;
    int64_t rows = 0;
    kr_stats stats;
};

// `spin`: as the Raytracer stores it (cartesian() squares it)
inline PathTimes record_paths_to_text(const kr_params& p, const kr_path_spec& w, bool write_cartesian, double spin, void* d_rays, int64_t n, const std::string& out_name)
{
    PathTimes tm;
    Stopwatch clock;
    DeviceBuffer d_offsets((n + 1) * (int64_t) sizeof(int64_t));
    DeviceBuffer d_traced(n);
    int64_t total = 0;
    check(kr_trace_paths_count_dev_f64(&p, &w, d_rays, n, d_offsets.get(), d_traced.get(), &total, nullptr), "count the path rows");
    tm.count_ms = clock.lap_ms();
    DeviceBuffer d_rows(total * 4 * (int64_t) sizeof(double));
    check(kr_trace_paths_record_dev_f64(&p, &w, d_rays, n, d_offsets.get(), d_rows.get(), total, nullptr, &tm.stats), "record the paths");
    tm.record_ms = clock.lap_ms();
    std::vector<int64_t> offsets((size_t) n + 1);
    std::vector<uint8_t> traced((size_t) n);
    PinnedDoubles rows(total * 4);
    check(kr_memcpy_d2h(offsets.data(), d_offsets.get(), (n + 1) * (int64_t) sizeof(int64_t)), "d2h offsets");
    check(kr_memcpy_d2h(traced.data(), d_traced.get(), n), "d2h traced");
    if (total > 0) check(kr_memcpy_d2h(rows.data(), d_rows.get(), total * 4 * (int64_t) sizeof(double)), "d2h rows");
    tm.readback_ms = clock.lap_ms();
    tm.rows = total;

    TextOutput outfile(out_name);
    for (int64_t i = 0; i < n; ++i) {
        if (!traced[(size_t) i]) continue;
        for (int64_t k = offsets[(size_t) i]; k < offsets[(size_t) i + 1]; ++k) {
            const double t = rows[4 * k], r = rows[4 * k + 1], theta = rows[4 * k + 2], phi = rows[4 * k + 3];
            if (write_cartesian) {
                double x, y, z;
                cartesian<double>(x, y, z, r, theta, phi, spin);
                outfile << t << x << y << z << endl;
            } else {
                outfile << t << r << theta << phi << endl;
            }
        }
        outfile.newline(2);
    }
    outfile.close();
    tm.text_ms = clock.lap_ms();
    return tm;
}

inline void print_path_times(const PathTimes& tm, double init_ms)
{
    std::cout << "timing: rays " << tm.stats.rays_traced << " steps " << tm.stats.steps_total << " rows " << tm.rows << " | init " << init_ms << " ms | count pass " << tm.count_ms
              << " ms | record pass " << tm.record_ms << " ms (kernel " << tm.stats.kernel_ms << ") | read-back " << tm.readback_ms << " ms | text file " << tm.text_ms << " ms"
              << std::endl;
}

}   // namespace krapp

#endif /* KR_APP_PATH_RECORDING_H_ */
