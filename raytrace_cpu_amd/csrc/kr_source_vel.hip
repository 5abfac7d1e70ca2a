// kr_source_vel.hip -- the point source with an arbitrary timelike four-velocity (kr_pointsource_vel_spec, include/kr_trace.h): the reference's
// PointSourceVel ctor (pointsource_vel.cpp:11-110) as a streaming kernel beside the trace.  The emitter's tetrad is solved ONCE PER LAUNCH on the host
// (kr_vel_tetrad.hpp: SolveTetrad, :113-260, operation for operation, C library sin / cos / tan of the one polar angle) and rides in the kernel
// arguments; the kernel is InitPointSourceVel (:34-110) against the 144-B AoS record, one ray per work-item, the record written with nine 16-byte
// stores.  acos of the grid's cos(alpha) is kr_crmath.hpp's correctly rounded routine, sin / cos of alpha and beta kr_sincos.hpp's; everything else is
// one IEEE operation under -ffp-contract=off in the reference's association -- tests/source_vel_rules.py restates the same rules in numpy and the
// device records must equal it bit for bit.
// Two departures from the reference, both in the header: an out-of-range grid point marks ONLY ITS OWN ray (steps = -1, the PointSource rule,
// pointsource.cpp:40-44) where :50 returns from the whole constructor; and the emitted energy is taken in the emitter's own frame, g_ab u^a p^b with
// the momentum the tetrad launched, where RedshiftStart(velocity) (:263-269) takes an orbital frame whatever the motion.

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "kr_pass.hpp"
#include "kr_crmath.hpp"
#include "kr_vel_tetrad.hpp"

namespace kr {

namespace {

// 144 bytes as nine 16-byte stores (records are 16-byte aligned: hipMalloc's alignment and a multiple of 16 per record)
KR_DEV void store_record(kr_ray_f64* dst, const kr_ray_f64& ray)
{
    static_assert(sizeof(kr_ray_f64) == 144, "nine double2 stores");
    double2 w[9];
    memcpy(w, &ray, sizeof(ray));
    double2* d = reinterpret_cast<double2*>(dst);
#pragma unroll
    for (int q = 0; q < 9; q++) d[q] = w[q];
}

// InitPointSourceVel for grid point ix = i n_beta + j; a slot beyond the grid or a point out of range is the Raytracer ctor's record (steps = -1)
template <bool EMIT>
KR_DEV kr_ray_f64 vel_ray(const kr_pointsource_vel_spec& s, const krvel::Frame& f, long long n_grid, int n_beta, long long ix)
{
    if (!(ix < n_grid)) return dead_ray();
    const int i = (int) (ix / n_beta), j = (int) (ix % n_beta);
    const double cosalpha = s.cosalpha0 + i * s.dcosalpha;
    const double beta = s.beta0 + j * s.dbeta;
    if (cosalpha >= s.cosalphamax || beta >= s.betamax) return dead_ray();

    kr_ray_f64 ray;
    memset(&ray, 0, sizeof(ray));
    ray.alpha = cosalpha;                         // sic: cos(alpha), as PointSource
    ray.beta = beta;
    ray.t = s.pos[0]; ray.r = s.pos[1]; ray.theta = s.pos[2]; ray.phi = s.pos[3];
    ray.steps = 0;

    const double alpha = krcr::kr_acos_cr(cosalpha);
    double sin_alpha, cos_alpha, sin_beta, cos_beta;
    kr_sincos_f64(alpha, sin_alpha, cos_alpha);
    kr_sincos_f64(beta, sin_beta, cos_beta);

    const double r = s.pos[1], a = s.spin, E = s.E;
    const double st = f.sin_th, ct = f.cos_th, tt = f.tan_th;
    const double rhosq = r * r + (a * ct) * (a * ct);

    const double rp0 = E, rp1 = E * sin_alpha * cos_beta, rp2 = E * sin_alpha * sin_beta, rp3 = E * cos_alpha;
    const double tdot = rp0 * f.tetrad[0][0] + rp1 * f.tetrad[1][0] + rp2 * f.tetrad[2][0] + rp3 * f.tetrad[3][0];
    const double rdot = rp0 * f.tetrad[0][1] + rp1 * f.tetrad[1][1] + rp2 * f.tetrad[2][1] + rp3 * f.tetrad[3][1];
    const double thetadot = rp0 * f.tetrad[0][2] + rp1 * f.tetrad[1][2] + rp2 * f.tetrad[2][2] + rp3 * f.tetrad[3][2];
    const double phidot = rp0 * f.tetrad[0][3] + rp1 * f.tetrad[1][3] + rp2 * f.tetrad[2][3] + rp3 * f.tetrad[3][3];

    const double k = (1 - 2 * r / rhosq) * tdot + (2 * a * r * st * st / rhosq) * phidot;
    double h = phidot * ((r * r + a * a) * (r * r + a * a * ct * ct - 2 * r) * st * st + 2 * a * a * r * st * st * st * st);
    h = h - 2 * a * r * k * st * st;
    h = h / (r * r + a * a * ct * ct - 2 * r);
    ray.k = k;
    ray.h = h;
    ray.Q = rhosq * rhosq * thetadot * thetadot - (a * k * ct + h / tt) * (a * k * ct - h / tt);
    ray.rdot_sign = (rdot > 0) ? 1 : -1;
    ray.thetadot_sign = (thetadot > 0) ? 1 : -1;
    if (EMIT) {
        // g_ab u^a p^b, the sixteen products in row-major order, zeros included (energy_dot, kr_post_device.hpp), u = u_in / sqrt(g(u_in, u_in))
        Metric<double> m;
        m.g00 = f.g00; m.g03 = f.g03; m.g11 = f.g11; m.g22 = f.g22; m.g33 = f.g33;
        const double p[4] = {tdot, rdot, thetadot, phidot};
        ray.emit = energy_dot<double>(m, f.un, p);
    }
    return ray;
}

template <bool EMIT>
__global__ void __launch_bounds__(kBlock)
pointsource_vel_init_kernel(kr_ray_f64* __restrict__ rays, long long n, kr_pointsource_vel_spec s, krvel::Frame f, int n_cosalpha, int n_beta)
{
    const long long n_grid = (long long) n_cosalpha * n_beta;
    KR_GRID_STRIDE(slot, n) store_record(&rays[slot], vel_ray<EMIT>(s, f, n_grid, n_beta, slot));
}

bool all_finite(const double* x, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(x[i])) return false;
    return true;
}

}  // namespace

// the ray count and the grid's factors as the reference's ctor truncates them (pointsource_vel.cpp:12, :15-16); false when the product is no int
bool pointsource_vel_grid(const kr_pointsource_vel_spec* s, int64_t* total, int* n_cosalpha, int* n_beta)
{
    const double fc = ((s->cosalphamax - s->cosalpha0) / s->dcosalpha) + 1;
    const double fb = ((s->betamax - s->beta0) / s->dbeta) + 1;
    const double prod = fc * fb;
    if (!(prod >= 0 && prod <= (double) INT_MAX && fc >= 0 && fc <= (double) INT_MAX && fb >= 0 && fb <= (double) INT_MAX)) return false;
    *total = (int) prod;
    *n_cosalpha = (int) fc;
    *n_beta = (int) fb;
    return true;
}

int pointsource_vel_validate(const kr_pointsource_vel_spec* s, const char* who, krvel::Frame* frame)
{
    if (!s) return invalid_arg(who, "null spec");
    if (!all_finite(s->pos, 4)) return invalid_arg(who, "pos is not finite");
    if (!all_finite(s->u, 4)) return invalid_arg(who, "u is not finite");
    if (!(s->pos[1] > 1 + std::sqrt((1 - s->spin) * (1 + s->spin)))) return invalid_arg(who, "the source lies on or inside the horizon (r <= horizon)");
    if (!(s->u[0] > 0)) return invalid_arg(who, "u^t must be positive");
    krvel::Frame f;
    krvel::solve_tetrad(s->pos, s->u, s->spin, &f);
    if (!(f.norm_u > 0)) return invalid_arg(who, "u is not timelike (g(u, u) <= 0)");
    int64_t total;
    int nc, nb;
    if (!pointsource_vel_grid(s, &total, &nc, &nb)) return invalid_arg(who, "the grid's ray count is not a non-negative int");
    if (frame) *frame = f;
    return KR_OK;
}

int pointsource_vel_init_dev(const kr_pointsource_vel_spec* s, const krvel::Frame* f, void* d, int64_t n, bool emit, hipStream_t st)
{
    if (n <= 0) return KR_OK;
    int64_t total;
    int nc, nb;
    pointsource_vel_grid(s, &total, &nc, &nb);
    const int grid = grid_for(n, kBlock, kCapStream);
    if (emit) hipLaunchKernelGGL(pointsource_vel_init_kernel<true>, dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *s, *f, nc, nb);
    else hipLaunchKernelGGL(pointsource_vel_init_kernel<false>, dim3(grid), dim3(kBlock), 0, st, (kr_ray_f64*) d, (long long) n, *s, *f, nc, nb);
    KR_LAUNCH_CHECK();
    return KR_OK;
}

}  // namespace kr
