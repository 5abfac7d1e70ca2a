// kr_pass.hpp -- what the O(N) passes either side of the trace kernel share (kr_post.hip, kr_return_map.hip, kr_line.hip, kr_spectrum.hip, kr_caustic.hip) and what kr_capi.hip calls
// them through: the launch helpers, the per-record pieces that several kernels repeat, and the one declaration of every launcher.
// kr_disc_pass.hpp (which includes this file) adds what the disc passes share among themselves: the disc filter, the per-ray front end, the tile compactor.
// The device helpers are plain forced-inline functions and one loop macro: each kernel compiles to the code it had with the lines written out.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

#include "kr_common.hpp"
#include "kr_post_device.hpp"
#include "kr_vel_tetrad.hpp"

namespace kr {

// ---- launching ---------------------------------------------------------------------------------------------------------------------------
constexpr int kBlock = 256;

// workgroups for `items` at `per_block` items each, at most `cap_blocks` (the kernels stride over the rest)
inline int grid_for(int64_t items, int per_block, int cap_blocks)
{
    const int64_t b = (items + per_block - 1) / per_block;
    return (int) std::max<int64_t>(1, std::min<int64_t>(b, cap_blocks));
}
constexpr int kCapStream = 256 * 16;       // streaming passes
constexpr int kCapHist = 256 * 4;          // few, fat workgroups: every workgroup flushes its whole LDS histogram, so keep the flush traffic below the ray traffic

#define KR_LAUNCH_CHECK() KR_HIP(hipGetLastError())

// kernel<true> with its histogram privatised in LDS (lds_bytes of dynamic LDS; 0 when the kernel sizes it statically) when it fits, else
// kernel<false> adding into the global histogram directly
#define KR_LAUNCH_LDS_OR_GLOBAL(kernel, fits, grid, lds_bytes, st, ...)                                   \
    do {                                                                                                  \
        if (fits) hipLaunchKernelGGL(kernel<true>, dim3(grid), dim3(kBlock), lds_bytes, st, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<false>, dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);             \
        KR_LAUNCH_CHECK();                                                                                \
    } while (0)

// ---- the disc flow of a launch (DiscFlow, kr_post_device.hpp) ------------------------------------------------------------------------------
// r_ms = kr_kerr_isco(a, +1) of the metric's a = reverse ? -spin : spin and the energy and angular momentum of the circular orbit there, every
// square root a double one (include/kr_trace.h, KR_V_PLUNGE)
inline DiscFlow<true> plunge_flow(double spin, int reverse)
{
    const double a = reverse ? -1 * spin : spin;
    DiscFlow<true> fl;
    fl.r_ms = kr_kerr_isco(a, +1);
    const double u = 1 / fl.r_ms;
    fl.E_ms = (1 - 2 * u + a * u * std::sqrt(u)) / std::sqrt(1 - 3 * u + 2 * a * u * std::sqrt(u));
    fl.L_ms = (1 + a * a * u * u - 2 * a * u * std::sqrt(u)) / std::sqrt(u * (1 - 3 * u + 2 * a * u * std::sqrt(u)));
    return fl;
}

// f(choice) with choice.plunge a compile-time bool and choice.arg the kernel's trailing DiscFlow argument: the plunge instance for V == KR_V_PLUNGE,
// today's instance for every other V
template <bool P> struct FlowChoice { static constexpr bool plunge = P; DiscFlow<P> arg; };
template <typename F>
void for_flow(double spin, double V, int reverse, F f)
{
    if (V == KR_V_PLUNGE) f(FlowChoice<true>{plunge_flow(spin, reverse)});
    else f(FlowChoice<false>{});
}

// KR_LAUNCH_LDS_OR_GLOBAL for kernel<USE_LDS, PLUNGE>(..., DiscFlow<PLUNGE>)
#define KR_LAUNCH_LDS_OR_GLOBAL_FLOW(kernel, spin, V, reverse, fits, grid, lds_bytes, st, ...)                             \
    do {                                                                                                                   \
        for_flow(spin, V, reverse, [&](auto flow_) {                                                                       \
            constexpr bool kPlunge_ = decltype(flow_)::plunge;                                                             \
            if (fits) hipLaunchKernelGGL((kernel<true, kPlunge_>), dim3(grid), dim3(kBlock), lds_bytes, st, __VA_ARGS__, flow_.arg); \
            else hipLaunchKernelGGL((kernel<false, kPlunge_>), dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__, flow_.arg);   \
        });                                                                                                                \
        KR_LAUNCH_CHECK();                                                                                                 \
    } while (0)

// Several small launches in one: the items of a chunk ride in the kernel arguments (no staging buffer whose lifetime a later call would have
// to track), blockIdx.y picks the item.  Chunk is struct { Item item[K]; }; fill(i, pins, &item) describes launch i (n[i] > 0; empty ones are
// skipped) and may pin device tables, which stay pinned until the chunk's launch is enqueued.  Blocks per item: block_budget over the items
// of the chunk but at least 64, never more than the largest item's rays need.
template <typename Chunk, typename Fill, typename Kernel, typename... Args>
int launch_chunked(int count, const int64_t* n, int block_budget, hipStream_t st, Fill fill, Kernel kernel, Args... args)
{
    constexpr int kChunk = (int) (sizeof(Chunk::item) / sizeof(Chunk::item[0]));
    for (int base = 0; base < count; base += kChunk) {
        Chunk c;
        std::memset(&c, 0, sizeof c);
        TablePins pins;
        int m = 0;
        int64_t n_max = 0;
        for (int i = base; i < count && i < base + kChunk; i++) {
            if (n[i] <= 0) continue;
            const int rc = fill(i, pins, &c.item[m++]);
            if (rc != KR_OK) return rc;
            n_max = std::max(n_max, n[i]);
        }
        if (m == 0) continue;
        const int per_item = (int) std::max<int64_t>(1, std::min<int64_t>((n_max + kBlock - 1) / kBlock, std::max(64, block_budget / m)));
        hipLaunchKernelGGL(kernel, dim3(per_item, m), dim3(kBlock), 0, st, c, args...);
        KR_LAUNCH_CHECK();
    }
    return KR_OK;
}

// ---- device side: one record / pixel per work-item ---------------------------------------------------------------------------------------
#define KR_GRID_STRIDE(i, n) for (long long i = blockIdx.x * (long long) kBlock + threadIdx.x; i < (n); i += (long long) gridDim.x * kBlock)

// the constants of motion and the end point that emit_value / redshift_value read, copied out of a record that the pass goes on to write to
template <typename R>
KR_DEV R geodesic_start_of(const R* ray)
{
    R v;
    v.r = ray->r; v.theta = ray->theta; v.k = ray->k; v.h = ray->h; v.Q = ray->Q; v.rdot_sign = ray->rdot_sign; v.thetadot_sign = ray->thetadot_sign;
    return v;
}

template <typename R>
KR_DEV R geodesic_of(const R* ray)
{
    R v = geodesic_start_of(ray);
    v.emit = ray->emit;
    return v;
}

// range_phi of one record: phi is written back only when wrapping changed it (NaN never is); returns the wrapped value
template <typename R, typename T>
KR_DEV T wrap_phi(R* ray, int steps, T lo, T hi)
{
    const T phi = ray->phi;
    const T wrapped = range_phi_value<T>(phi, steps, lo, hi);
    if (!(wrapped == phi) && wrapped == wrapped) ray->phi = wrapped;
    return wrapped;
}

// ---- launchers (device pointers; the stream may be null) and validators behind the C API ---------------------------------------------------
// kr_post.hip.  f32: the records are kr_ray_f32 and the pass computes in float (the scalars are float values carried in doubles)
int redshift_start_dev(double spin, double V, int reverse, int projradius, void* d, int64_t n, hipStream_t st, bool f32);
int redshift_dev(double spin, double V, int reverse, int projradius, int motion, void* d, int64_t n, hipStream_t st, bool f32);
int redshift_dest_dev(double spin, int reverse, void* d, int64_t n, hipStream_t st, bool f32);
int range_phi_dev(double lo, double hi, void* d, int64_t n, hipStream_t st, bool f32);
int calculate_momentum_dev(double spin, void* d, int64_t n, hipStream_t st, bool f32);
int pointsource_init_dev(const kr_pointsource* s, void* d, int64_t n, int64_t first, int64_t stride, hipStream_t st);
int pointsource_init_emit_dev(const kr_pointsource* s, void* d, int64_t n, int64_t first, int64_t stride, double V, int reverse, int projradius, hipStream_t st);
int pointsource_init_emit_batch_dev(int count, const kr_pointsource* s, const double* V, int reverse, int projradius, void* const* d, const int64_t* n, hipStream_t st);
PlaneTrig plane_trig(const kr_imageplane* s);
int imageplane_init_dev(const kr_imageplane* s, void* d, int64_t n, int64_t first, int64_t stride, hipStream_t st);
int imageplane_init_emit_dev(const kr_imageplane* s, void* d, int64_t n, int64_t first, int64_t stride, int64_t run, double spin, double V, int reverse,
                             int projradius, hipStream_t st);
int reduce_emissivity_dev(const kr_emis_bins* b, const void* d, int64_t n, void* d_hist, hipStream_t st);
int post_emissivity_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_emis_bins* b, void* d, int64_t n,
                        void* d_hist, hipStream_t st);
int reduce_image_dev(const kr_image_bins* b, const void* d, int64_t n, void* d_planes, hipStream_t st);
int post_image_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_image_bins* b, void* d, int64_t n,
                   void* d_planes, hipStream_t st);
int reduce_return_dev(const kr_return_bins* b, const void* d, int64_t n, void* d_out4, hipStream_t st);
int post_return_dev(double lo, double hi, const kr_return_bins* b, void* d, int64_t n, void* d_out4, hipStream_t st);
int post_return_batch_dev(int count, double lo, double hi, const kr_return_bins* b, void* const* d, const int64_t* n, void* const* d_out4, hipStream_t st);
int arith_probe_dev(int op, const double* a, const double* b, double* out, int64_t n);
// kr_surface.hip: the emissivity histogram and the image of rays that ended on a stop surface (KR_STATUS_DEST), binned by rho = r sin(theta); the
// post_ forms take the Keplerian observer at rho, redshift(V = -1, projradius = 1, motion = 0)
int reduce_emissivity_surface_dev(const kr_emis_bins* b, const void* d, int64_t n, void* d_hist, hipStream_t st);
int post_emissivity_surface_dev(double spin, int reverse, double lo, double hi, const kr_emis_bins* b, void* d, int64_t n, void* d_hist, hipStream_t st);
int reduce_image_surface_dev(const kr_image_bins* b, const void* d, int64_t n, void* d_planes, hipStream_t st);
int post_image_surface_dev(double spin, int reverse, double lo, double hi, const kr_image_bins* b, void* d, int64_t n, void* d_planes, hipStream_t st);
// the line, the continuum and the response of rays that landed on the surface of a kr_disc_surface (kr_line.hip, kr_spectrum.hip, kr_response.hip;
// the per-record angles: kr_angles.hip).  surface_validate (kr_surface.hip) refuses a null surface and what KR_STOP_THICKDISC refuses of its stop_params
int surface_validate(const kr_disc_surface* s, const char* who);
int angles_surface_dev(const kr_disc_surface* s, double spin, int reverse, const void* d, int64_t n, void* d_angles, hipStream_t st);
int post_line_surface_dev(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law, void* d, int64_t n,
                          void* d_line, hipStream_t st);
int reduce_line_surface_dev(const kr_line_bins* b, const void* d, int64_t n, void* d_line, hipStream_t st);
int post_spectrum_surface_dev(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_spectrum_model* m, const kr_limb_law* law, void* d,
                              int64_t n, void* d_out, hipStream_t st);
int reduce_spectrum_surface_dev(const kr_spectrum_model* m, const void* d, int64_t n, void* d_out, hipStream_t st);
int post_response_surface_dev(const kr_disc_surface* s, double spin, int reverse, double lo, double hi, const kr_response_model* r, const kr_limb_law* law, void* d,
                              int64_t n, void* d_out, hipStream_t st);
int reduce_response_surface_dev(const kr_response_model* r, const void* d, int64_t n, void* d_out, hipStream_t st);
// kr_return_map.hip: the landing map of the returning radiation (kr_return_map); the validator refuses a null map and nr <= 0
int return_map_validate(const kr_return_map* m, const char* who);
int reduce_return_map_dev(const kr_return_map* m, const void* d, int64_t n, void* d_out, hipStream_t st);
int post_return_map_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_return_map* m, void* d, int64_t n, void* d_out,
                        hipStream_t st);
int post_return_map_batch_dev(int count, double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_return_map* m, void* const* d,
                              const int64_t* n, void* const* d_out, hipStream_t st);
// kr_healpix.hip: the HEALPix point source (kr_healpix_source) and the fate map of its sky (kr_healpix_map).  The validators refuse what the structs'
// comments refuse and a shard that reaches beyond the sphere; first / stride count pixels
int healpix_validate(const kr_healpix_source* s, const char* who);
int healpix_shard_validate(const kr_healpix_source* s, int64_t first, int64_t stride, int64_t count, const char* who);
int healpix_vectors_validate(int order, int64_t first, int64_t stride, int64_t count, const char* who);
int healpix_map_validate(const kr_healpix_map* m, int64_t n, int64_t first, int64_t stride, const char* who);
int healpix_vectors_dev(int order, int unit_center, int64_t first, int64_t stride, int64_t count, void* d_out, hipStream_t st);
int healpix_init_dev(const kr_healpix_source* s, void* d, int64_t n, int64_t first, int64_t stride, bool emit, int reverse, hipStream_t st);
int reduce_healpix_map_dev(const kr_healpix_map* m, const void* d, int64_t n, int64_t first, int64_t stride, void* d_out, hipStream_t st);
int post_healpix_map_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_healpix_map* m, void* d, int64_t n, int64_t first,
                         int64_t stride, void* d_out, hipStream_t st);
// kr_line.hip
int line_validate(const kr_line_bins* b, const char* who);
int reduce_line_dev(const kr_line_bins* b, const void* d, int64_t n, void* d_line, hipStream_t st);
int post_line_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_line_bins* b, void* d, int64_t n,
                  void* d_line, hipStream_t st);
int line_from_image_dev(const kr_line_bins* b, const kr_image_bins* ib, const void* d_planes, void* d_line, hipStream_t st);
int post_line_limb_dev(double spin, double V, int reverse, int projradius, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law, void* d, int64_t n,
                       void* d_line, hipStream_t st);
// kr_spectrum.hip: the continuum spectrum (kr_spectrum_model); the validators refuse what the struct's comment refuses, a bad limb law, and motion != 0
// with a law other than 0
int spectrum_validate(const kr_spectrum_model* m, const char* who);
int spectrum_law_validate(const kr_limb_law* law, int motion, const char* who);
int post_spectrum_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_spectrum_model* m, const kr_limb_law* law, void* d,
                      int64_t n, void* d_out, hipStream_t st);
int reduce_spectrum_dev(const kr_spectrum_model* m, const void* d, int64_t n, void* d_out, hipStream_t st);
// the Stokes spectra (STOKES SPECTRA under kr_spectrum_model): motion 0 only; the reduce form recomputes the frame of the on-disc records
int post_spectrum_stokes_dev(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_spectrum_model* m, const kr_limb_law* law,
                             const kr_pol_law* pol, void* d, int64_t n, void* d_out, hipStream_t st);
int reduce_spectrum_stokes_dev(double spin, double V, int reverse, int projradius, double inc_deg, const kr_spectrum_model* m, const kr_limb_law* law, const kr_pol_law* pol,
                               const void* d, int64_t n, void* d_out, hipStream_t st);
// kr_response.hip: the energy-time response of the reflection spectrum (kr_response_model); the validator refuses what spectrum_validate refuses of
// spec, then what the struct's comment refuses (the limb law: spectrum_law_validate)
int response_validate(const kr_response_model* r, const char* who);
int post_response_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_response_model* r, const kr_limb_law* law, void* d,
                      int64_t n, void* d_out, hipStream_t st);
int reduce_response_dev(const kr_response_model* r, const void* d, int64_t n, void* d_out, hipStream_t st);
// kr_hotspot.hip: the orbiting hot spot (kr_hotspot); the validator refuses what the struct's comment refuses (the limb law: spectrum_law_validate)
int hotspot_validate(const kr_hotspot* h, const char* who);
int post_hotspot_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_hotspot* h, const kr_limb_law* law, void* d, int64_t n,
                     void* d_out, hipStream_t st);
int reduce_hotspot_dev(const kr_hotspot* h, const void* d, int64_t n, void* d_out, hipStream_t st);
// the Stokes light curves of the spot (the Stokes rule under kr_hotspot): motion 0 only; the reduce form recomputes the frame of the ring records
int post_hotspot_stokes_dev(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_hotspot* h, const kr_limb_law* law,
                            const kr_pol_law* pol, void* d, int64_t n, void* d_out, hipStream_t st);
int reduce_hotspot_stokes_dev(double spin, double V, int reverse, int projradius, double inc_deg, const kr_hotspot* h, const kr_limb_law* law, const kr_pol_law* pol,
                              const void* d, int64_t n, void* d_out, hipStream_t st);
// kr_angles.hip: the photon's angles in the disc frame (the observer of redshift_dev with motion 0; the validators refuse any other motion, a bad
// limb law, and nr < 1 or nmu < 1)
int angles_validate(int motion, const char* who);
int limb_validate(const kr_limb_law* law, const char* who);
int emissivity_mu_validate(const kr_emis_bins* b, const kr_mu_bins* mb, const char* who);
int angles_dev(double spin, double V, int reverse, int projradius, const void* d, int64_t n, void* d_angles, hipStream_t st);
int post_emissivity_mu_dev(double spin, double V, int reverse, int projradius, double lo, double hi, const kr_emis_bins* b, const kr_mu_bins* mb, void* d, int64_t n,
                           void* d_hist, void* d_mu, hipStream_t st);
// kr_polarisation.hip: the polarisation of disc emission on an image plane (the validators refuse reverse != 1, motion != 0, a non-finite inclination
// and a bad pol law); the Stokes line lives in kr_line.hip
int polarisation_validate(int reverse, int motion, double inc_deg, const char* who);
int pol_validate(const kr_pol_law* law, const char* who);
double sin_inclination(double inc_deg);
int polarisation_dev(double spin, double V, int reverse, int projradius, double inc_deg, const void* d, int64_t n, void* d_out, hipStream_t st);
int post_image_stokes_dev(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_image_bins* b, const kr_limb_law* limb,
                          const kr_pol_law* pol, void* d, int64_t n, void* d_stokes, hipStream_t st);
int post_line_stokes_dev(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_line_bins* b, const kr_limb_law* limb,
                         const kr_pol_law* pol, void* d, int64_t n, void* d_out, hipStream_t st);
// kr_source_vel.hip: the point source with an arbitrary four-velocity.  The validator refuses what kr_pointsource_vel_spec's comment refuses and hands
// back the emitter's frame (kr_vel_tetrad.hpp), solved on the host; the grid helper gives the reference's truncated counts (false: no int)
bool pointsource_vel_grid(const kr_pointsource_vel_spec* s, int64_t* total, int* n_cosalpha, int* n_beta);
int pointsource_vel_validate(const kr_pointsource_vel_spec* s, const char* who, krvel::Frame* frame);
int pointsource_vel_init_dev(const kr_pointsource_vel_spec* s, const krvel::Frame* f, void* d, int64_t n, bool emit, hipStream_t st);
// kr_angdist.hip: where a source's rays end, by emission angle; the validator refuses a null spec and a dangle that gives no 1 ... 4096 bins
int angdist_nangle(const kr_angdist_spec* sp);
int angdist_validate(const kr_angdist_spec* sp, const char* who);
int reduce_angdist_dev(const kr_angdist_spec* sp, const void* d, int64_t n, void* d_out, hipStream_t st);
int post_angdist_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_angdist_spec* sp, void* d, int64_t n, void* d_out,
                     hipStream_t st);
// kr_observer.hip: the source-to-observer link; the validator refuses what kr_observer_spec's comment refuses of the spec; observer_words:
// nmu (4 + nt) + 10 of a spec that passed
int observer_validate(const kr_observer_spec* sp, const char* who);
int64_t observer_words(const kr_observer_spec* sp);
int reduce_observer_dev(const kr_observer_spec* sp, const void* d, int64_t n, void* d_out, hipStream_t st);
int post_observer_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_observer_spec* sp, void* d, int64_t n, void* d_out,
                      hipStream_t st);
// kr_illum.hip: the (r, phi) illumination map; the validator refuses what kr_illum_bins' comment refuses of the bins; illum_words: 5 nr nphi + 2 of
// bins that passed
int illum_validate(const kr_illum_bins* m, const char* who);
int64_t illum_words(const kr_illum_bins* m);
int reduce_illum_dev(const kr_illum_bins* m, const void* d, int64_t n, void* d_out, hipStream_t st);
int post_illum_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_illum_bins* m, void* d, int64_t n, void* d_out,
                   hipStream_t st);
// the line and the response with an (r, phi) illumination table (kr_line.hip, kr_response.hip); the validator (kr_illum.hip) refuses what
// kr_illum_table's comment refuses of the table itself
int illum_table_validate(const kr_illum_table* t, const char* who);
int post_line_illum_dev(double spin, double V, int reverse, int projradius, double lo, double hi, const kr_line_bins* b, const kr_limb_law* law, const kr_illum_table* t,
                        void* d, int64_t n, void* d_line, hipStream_t st);
int reduce_line_illum_dev(const kr_line_bins* b, const kr_illum_table* t, const void* d, int64_t n, void* d_line, hipStream_t st);
int post_response_illum_dev(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_response_model* r, const kr_limb_law* law,
                            const kr_illum_table* t, void* d, int64_t n, void* d_out, hipStream_t st);
int reduce_response_illum_dev(const kr_response_model* r, const kr_illum_table* t, const void* d, int64_t n, void* d_out, hipStream_t st);
// kr_caustic.hip.  The validators take the records the caller has (n; "n smaller than ..." is theirs to say)
int caustic_validate(const kr_caustic_map* m, int64_t n, const char* who);
int bundles_init_emit_dev(const kr_imageplane* s, int nx, int ny, double eps_frac, double V, int reverse, int projradius, void* d, int64_t n, hipStream_t st);
int post_caustic_dev(double spin, int reverse, const kr_caustic_map* m, void* d, int64_t n, void* d_maps, hipStream_t st);
int caustic_suppress_dev(const kr_caustic_map* m, void* d_maps, hipStream_t st);
int source_map_validate(const kr_source_map* m, int64_t n, const char* who);
int post_caustic_source_dev(const kr_source_map* m, const void* d, void* d_maps, hipStream_t st);
// kr_paths.hip: the two passes of the recording trace; both wait for `st` (the count pass hands the total to the host, the record pass its verdict)
int paths_validate(const kr_params* p, const kr_path_spec* w, const char* who);
int paths_count_dev(const kr_params* p, const kr_path_spec* w, const void* d_rays, int64_t n, void* d_offsets, void* d_traced, int64_t* total_rows, hipStream_t st);
int paths_record_dev(const kr_params* p, const kr_path_spec* w, void* d_rays, int64_t n, const void* d_offsets, void* d_rows, int64_t total_rows, hipStream_t st,
                     kr_stats* stats);
// kr_volume.hip: the mapping trace; the validator refuses a bad grid and what paths_validate refuses of the params; the launcher waits for `st`
int volume_validate(const kr_params* p, const kr_volume_map* m, const char* who);
int trace_volume_dev(const kr_params* p, const kr_volume_map* m, void* d_rays, int64_t n, void* d_map, hipStream_t st, kr_stats* stats);
// kr_observe.hip: the observing trace; the validator refuses what volume_validate refuses, then bad bins; the launcher waits for `st`
int observe_validate(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const char* who);
int trace_observe_dev(const kr_params* p, const kr_volume_map* m, const kr_observe_bins* b, const void* d_emis, const void* d_kappa, const void* d_delay, void* d_rays,
                      int64_t n, void* d_out, void* d_image, hipStream_t st, kr_stats* stats);
// kr_crossings.hip: the crossing-recording trace; the validator refuses a bad spec and what paths_validate refuses of the params; the launcher waits
// for `st`.  kr_post.hip: the image of one order from what it recorded
int crossings_validate(const kr_params* p, const kr_crossing_spec* sp, const char* who);
int trace_crossings_dev(const kr_params* p, const kr_crossing_spec* sp, void* d_rays, int64_t n, void* d_rows, void* d_seen, hipStream_t st, kr_stats* stats);
int reduce_crossing_image_dev(const kr_image_bins* b, int max_crossings, int order, double lo, double hi, const void* d_rays, const void* d_rows, const void* d_seen,
                              int64_t n, void* d_planes, hipStream_t st);

}  // namespace kr
