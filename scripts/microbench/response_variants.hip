// response_variants.hip -- raytrace_cpu_amd/csrc/kr_response.hip itself, compiled again with its A/B switches, for scripts/response_ab.py only:
//   -DKR_RESPONSE_SORT=0    leave a tile's items in traced order (the library orders them by time row in LDS before phase B)
//   -DKR_RESPONSE_CHUNK=0   the grid-stride tiles of kr_spectrum.hip (in the library a workgroup takes a contiguous run of tiles)
// Built as a small shared library next to this file and linked against libkrtrace.so for the host-side plumbing (the table store, spectrum_dev, set_error):
//   hipcc --offload-arch=gfx950 <the flags of _build.py> -D... -shared -Wl,-Bsymbolic -o libresponse_<tag>.so response_variants.hip -L<csrc> -lkrtrace
#include "../../raytrace_cpu_amd/csrc/kr_response.hip"

extern "C" int variant_post_response(double spin, double V, int reverse, int projradius, int motion, double lo, double hi, const kr_response_model* r, const kr_limb_law* law,
                                     void* d_rays, long long n, void* d_out)
{
    return kr::post_response_dev(spin, V, reverse, projradius, motion, lo, hi, r, law, d_rays, n, d_out, nullptr);
}

extern "C" int variant_reduce_response(const kr_response_model* r, const void* d_rays, long long n, void* d_out)
{
    return kr::reduce_response_dev(r, d_rays, n, d_out, nullptr);
}
