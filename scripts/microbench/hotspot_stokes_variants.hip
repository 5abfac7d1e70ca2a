// hotspot_stokes_variants.hip -- raytrace_cpu_amd/csrc/kr_hotspot.hip itself, compiled again with one of the A/B switches of its Stokes instances, for
// scripts/hotspot_stokes_ab.py only:
//   -DKR_HOTSPOT_STOKES_POLAR_ALL               the fused form takes polar_value for every record instead of frame_value for every record and
//                                               polar_value for the ring survivors
//   -DKR_HOTSPOT_STOKES_TWO_WAVE_SLOTS=<N>      hold the Stokes kernels to two waves per SIMD up to N slots (0: never, the compiler sizes them)
//   -DKR_HOTSPOT_STOKES_TWO_WAVE_MIN_SLOTS=<N>  ... and from N slots: 1, at one slot in every form; 2, in none (the library: at one slot in the fused forms and
//                                               in the reduce forms with a spectrogram)
// Built as a small shared library next to this file and linked against libkrtrace.so for the host-side plumbing (set_error, hip_fail, sin_inclination):
//   hipcc --offload-arch=gfx950 <the flags of _build.py> -D... -shared -Wl,-Bsymbolic -o libhotspot_stokes_<tag>.so hotspot_stokes_variants.hip -L<csrc> -lkrtrace
#include "../../raytrace_cpu_amd/csrc/kr_hotspot.hip"

extern "C" int variant_post_hotspot_stokes(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_hotspot* h,
                                           const kr_limb_law* law, const kr_pol_law* pol, void* d_rays, long long n, void* d_out)
{
    return kr::post_hotspot_stokes_dev(spin, V, reverse, projradius, lo, hi, inc_deg, h, law, pol, d_rays, n, d_out, nullptr);
}

extern "C" int variant_reduce_hotspot_stokes(double spin, double V, int reverse, int projradius, double inc_deg, const kr_hotspot* h, const kr_limb_law* law,
                                             const kr_pol_law* pol, const void* d_rays, long long n, void* d_out)
{
    return kr::reduce_hotspot_stokes_dev(spin, V, reverse, projradius, inc_deg, h, law, pol, d_rays, n, d_out, nullptr);
}
