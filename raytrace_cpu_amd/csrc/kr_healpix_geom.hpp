// kr_healpix_geom.hpp -- the pixel geometry of the HEALPix point source (include/kr_trace.h, kr_healpix_source: "geometry"), ONE definition for the
// device source (kr_healpix.hip) and for the host class mirror (host/raytracer/healpix_pointsource.h).  RING pixel -> position on one of the twelve
// base faces -> the four corner directions and their average.  The arithmetic is the reference's healpix.h, value for value (32-bit integers, its
// integer square root through a double, its association, its fixed rotation of 0.05 in azimuth, the un-normalised centre); the caller supplies
// the sin / cos pair through `Math` -- the strict trace's correctly rounded pair on the device, the C library on the host -- everything else is
// a single IEEE operation, so build with -ffp-contract=off.
#pragma once

#if defined(__HIPCC__)
#define KR_HPX_FN __host__ __device__ inline
#else
#define KR_HPX_FN inline
#endif

namespace krhpx {

KR_HPX_FN double root(double x) { return __builtin_sqrt(x); }
KR_HPX_FN float root(float x) { return __builtin_sqrtf(x); }

// row and column offsets of the twelve base faces: {2,2,2,2,3,3,3,3,4,4,4,4} and {1,3,5,7,0,2,4,6,1,3,5,7}, as two shift expressions a lane need not index
KR_HPX_FN int face_row(int face) { return 2 + (face >> 2); }
KR_HPX_FN int face_col(int face) { return 2 * (face & 3) + ((face >> 2) != 1 ? 1 : 0); }

// the ring of a polar cap that holds count n: (1 + isqrt(n)) / 2 with isqrt(n) = (int) sqrt(n + 0.5) in double
KR_HPX_FN int cap_ring(int n) { return (1 + (int) root(n + 0.5)) >> 1; }

struct FacePos { int ix, iy, face; };

// where RING pixel `pix` of a sphere of 12 * 4^order pixels lies: base face and integer position on it
KR_HPX_FN FacePos face_position(int order, int pix)
{
    const int side = 1 << order, side2 = 2 * side, per_face = side << order, cap = (per_face - side) << 1, total = 12 * per_face;
    int ring, in_ring, shift, ring_len, face;        // ring from the north pole, 1-based place in it, half-pixel shift, pixels per quarter ring
    if (pix < cap) {                                 // northern cap
        ring = cap_ring(1 + 2 * pix);
        in_ring = (pix + 1) - 2 * ring * (ring - 1);
        shift = 0;
        ring_len = ring;
        face = (in_ring - 1) / ring_len;
    } else if (pix < total - cap) {                  // belt
        const int k = pix - cap;
        const int row = k >> (order + 2);
        ring = row + side;
        in_ring = k - row * 4 * side + 1;
        shift = (ring + side) & 1;
        ring_len = side;
        const int down = ring - side + 1, up = side2 + 2 - down;
        const int fa = (in_ring - down / 2 + side - 1) >> order, fb = (in_ring - up / 2 + side - 1) >> order;
        face = (fb == fa) ? (fb | 4) : ((fb < fa) ? fb : (fa + 8));
    } else {                                         // southern cap
        const int k = total - pix;
        const int from_south = cap_ring(2 * k - 1);
        in_ring = 4 * from_south + 1 - (k - 2 * from_south * (from_south - 1));
        shift = 0;
        ring_len = from_south;
        ring = 2 * side2 - from_south;
        face = 8 + (in_ring - 1) / ring_len;
    }
    const int v = ring - face_row(face) * side;
    int hz = 2 * in_ring - face_col(face) * ring_len - shift - 1;
    if (hz >= side2) hz -= 8 * side;
    FacePos p;
    p.ix = (hz - v) >> 1;
    p.iy = (-hz - v) >> 1;
    p.face = face;
    return p;
}

// the direction of the point (x, y) of a base face
template <typename Math, typename T>
KR_HPX_FN void face_direction(T x, T y, int face, T* vec)
{
    const T band = face_row(face) - x - y;           // < 1: northern cap, > 3: southern cap, else the belt
    T width, z;
    if (band < 1) {
        width = band;
        const T w2 = width * width / 3.;
        z = 1 - w2;
    } else if (band > 3) {
        width = 4 - band;
        const T w2 = width * width / 3.;
        z = w2 - 1;
    } else {
        width = 1;
        z = (2 - band) * 2. / 3.;
    }
    T turn = face_col(face) * width + x - y;         // azimuth in eighths of a turn, brought into [0, 8)
    if (turn < 0) turn += 8;
    if (turn >= 8) turn -= 8;
    const T phi = (width < 1e-15) ? 0 : (0.25 * 3.14159265358979323846 * turn) / width;
    const T sin_theta = root((1.0 - z) * (1.0 + z));
    T s, c;
    Math::sincos(phi + 0.05, s, c);
    vec[0] = sin_theta * c;
    vec[1] = sin_theta * s;
    vec[2] = z;
}

// centre and half width of a pixel on its face
template <typename T>
struct PixelFrame { T xc, yc, half; int face; };

template <typename T>
KR_HPX_FN PixelFrame<T> pixel_frame(int order, int pix)
{
    const FacePos p = face_position(order, pix);
    const int side = 1 << order;
    PixelFrame<T> f;
    f.half = 0.5 / side;
    f.xc = (p.ix + 0.5) / side;
    f.yc = (p.iy + 0.5) / side;
    f.face = p.face;
    return f;
}

// corner i: (xc + half, yc + half), (xc - half, yc + half), (xc - half, yc - half), (xc + half, yc - half)
template <typename Math, typename T>
KR_HPX_FN void pixel_corner(const PixelFrame<T>& f, int i, T* vec)
{
    const T x = (i == 0 || i == 3) ? f.xc + f.half : f.xc - f.half;
    const T y = (i < 2) ? f.yc + f.half : f.yc - f.half;
    face_direction<Math, T>(x, y, f.face, vec);
}

// the centre from the four corners: summed left to right, not normalised unless `unit`
template <typename T>
KR_HPX_FN void pixel_centre(const T* corners, int unit, T* centre)
{
    for (int c = 0; c < 3; c++) centre[c] = 0.25 * (corners[c] + corners[3 + c] + corners[6 + c] + corners[9 + c]);
    if (unit) {
        const T len = root(centre[0] * centre[0] + centre[1] * centre[1] + centre[2] * centre[2]);
        centre[0] = centre[0] / len; centre[1] = centre[1] / len; centre[2] = centre[2] / len;
    }
}

// all fifteen components of a pixel: four corners, then the centre
template <typename Math, typename T>
KR_HPX_FN void pixel_vectors(int order, int pix, int unit, T* v)
{
    const PixelFrame<T> f = pixel_frame<T>(order, pix);
    for (int c = 0; c < 4; c++) pixel_corner<Math, T>(f, c, &v[3 * c]);
    pixel_centre<T>(v, unit, &v[12]);
}

}  // namespace krhpx
