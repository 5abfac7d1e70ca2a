// tests/golden/healpix_vectors_dump.cpp -- fixture generator (build machine only): the pixel vectors that the REFERENCE's healpix.h computes, dumped
// as raw records {int32 order, int32 pix, double[15]: four corners then the centre}.  The reference's header is included where it lies
// (make_healpix_golden.sh passes -I<reference>/src/include); nothing of its text is copied here.  The pixels: every pixel of orders 0-3, and at orders
// 8 and 12 a sample of 512 -- the six pixels either side of the cap / belt boundaries and the ends, the first and last pixel of 64 rings spread over
// the sphere, and pixels at a fixed stride for the rest.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <set>

using namespace std;
#include "healpix.h"

static void dump(FILE* f, int order, int pix)
{
    double v[15];
    get_pixel_vectors<double>(order, pix, v, v + 12);
    int32_t head[2] = {order, pix};
    fwrite(head, sizeof head, 1, f);
    fwrite(v, sizeof v, 1, f);
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s out.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "wb");
    if (!f) return 1;
    for (int order = 0; order <= 3; order++)
        for (int pix = 0; pix < 12 * (1 << order) * (1 << order); pix++) dump(f, order, pix);
    const int sampled[2] = {8, 12};
    for (int order : sampled) {
        const long long nside = 1LL << order, npix = 12 * nside * nside, ncap = 2 * nside * (nside - 1);
        set<long long> pick = {0, ncap - 1, ncap, npix - ncap - 1, npix - ncap, npix - 1};
        const long long nrings = 4 * nside - 1;
        for (int q = 0; q < 64; q++) {
            const long long i = 1 + q * (nrings - 1) / 63;            // ring, counted from the north pole
            long long first, last;
            if (i < nside) { first = 2 * i * (i - 1); last = 2 * i * (i + 1) - 1; }
            else if (i <= 3 * nside) { first = ncap + (i - nside) * 4 * nside; last = first + 4 * nside - 1; }
            else { const long long j = 4 * nside - i; first = npix - 2 * j * (j + 1); last = npix - 2 * j * (j - 1) - 1; }
            pick.insert(first);
            pick.insert(last);
        }
        for (long long k = 1; pick.size() < 512; k++) pick.insert((k * 2654435761LL) % npix);
        for (long long pix : pick) dump(f, order, (int) pix);
    }
    fclose(f);
    return 0;
}
