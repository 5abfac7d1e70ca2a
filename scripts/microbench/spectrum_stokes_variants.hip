// spectrum_stokes_variants.hip -- raytrace_cpu_amd/csrc/kr_spectrum.hip itself, compiled again with one of the A/B switches of its Stokes instances, for
// scripts/spectrum_stokes_ab.py only:
//   -DKR_SPECTRUM_STOKES_FRAME_FIRST            the fused form takes frame_value for every record and polar_value for the on-disc ones (the library:
//                                               polar_value for every record in place of frame_value)
//   -DKR_SPECTRUM_STOKES_TWO_WAVE_SLOTS=<N>     hold EVERY Stokes kernel to two waves per SIMD up to N slots (0: none, the compiler sizes them all; the
//                                               library: only the fused table forms at four slots)
// Built as a small shared library next to this file and linked against libkrtrace.so for the host-side plumbing (set_error, the table store, sin_inclination):
//   hipcc --offload-arch=gfx950 <the flags of _build.py> -D... -shared -Wl,-Bsymbolic -o libspectrum_stokes_<tag>.so spectrum_stokes_variants.hip -L<csrc> -lkrtrace
#include "../../raytrace_cpu_amd/csrc/kr_spectrum.hip"

extern "C" int variant_post_spectrum_stokes(double spin, double V, int reverse, int projradius, double lo, double hi, double inc_deg, const kr_spectrum_model* m,
                                            const kr_limb_law* law, const kr_pol_law* pol, void* d_rays, long long n, void* d_out)
{
    return kr::post_spectrum_stokes_dev(spin, V, reverse, projradius, lo, hi, inc_deg, m, law, pol, d_rays, n, d_out, nullptr);
}

extern "C" int variant_reduce_spectrum_stokes(double spin, double V, int reverse, int projradius, double inc_deg, const kr_spectrum_model* m, const kr_limb_law* law,
                                              const kr_pol_law* pol, const void* d_rays, long long n, void* d_out)
{
    return kr::reduce_spectrum_stokes_dev(spin, V, reverse, projradius, inc_deg, m, law, pol, d_rays, n, d_out, nullptr);
}
