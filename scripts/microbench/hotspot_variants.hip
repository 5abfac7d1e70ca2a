// hotspot_variants.hip -- raytrace_cpu_amd/csrc/kr_hotspot.hip itself, compiled again with one of its A/B switches, for scripts/hotspot_ab.py only:
//   -DKR_HOTSPOT_SPARSE_MIN_SLOTS=<N>   the sparsity test from N slots per lane (99: never, every (item, sample) pair takes the cosine; 1: always)
//   -DKR_HOTSPOT_SPEC_LDS_WORDS=<N>     another LDS budget of the spectrogram block (0: always global adds)
//   -DKR_HOTSPOT_TWO_WAVE_SLOTS=<N>     hold the kernels to two waves per SIMD up to N slots (0: never, the compiler sizes them)
//   -DKR_HOTSPOT_TWO_WAVE_MIN_SLOTS=<N> ... and from N slots (the library: 2; 1: at one slot too)
// Built as a small shared library next to this file and linked against libkrtrace.so for the host-side plumbing (set_error, hip_fail):
//   hipcc --offload-arch=gfx950 <the flags of _build.py> -D... -shared -Wl,-Bsymbolic -o libhotspot_<tag>.so hotspot_variants.hip -L<csrc> -lkrtrace
#include "../../raytrace_cpu_amd/csrc/kr_hotspot.hip"

extern "C" int variant_post_hotspot(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_hotspot* h, const kr_limb_law* law,
                                    void* d_rays, long long n, void* d_out)
{
    return kr::post_hotspot_dev(spin, V, reverse, projradius, motion, lo, hi, h, law, d_rays, n, d_out, nullptr);
}

extern "C" int variant_reduce_hotspot(const kr_hotspot* h, const void* d_rays, long long n, void* d_out)
{
    return kr::reduce_hotspot_dev(h, d_rays, n, d_out, nullptr);
}
