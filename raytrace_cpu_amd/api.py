"""Thin Python conveniences over the C ABI (include/kr_trace.h): numpy in, numpy out.

Every function goes through libkrtrace.so (HIP, gfx950).  Nothing here computes on the CPU and nothing
falls back: if the library is missing or no GPU is visible the call raises KrError.
"""
import ctypes as C
import math

import numpy as np

from . import capi
from .capi import KrError, Params, Stats  # noqa: F401
from .devmem import DeviceScope

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = capi.load()
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _rays_arg(rays, dtype):
    if not isinstance(rays, np.ndarray) or rays.dtype != dtype or not rays.flags["C_CONTIGUOUS"]:
        raise KrError(f"rays must be a C-contiguous numpy array of dtype {dtype.names and 'Ray' or dtype}")
    return rays


def device_count():
    n = lib().kr_device_count()
    if n < 0:
        raise KrError(lib().kr_last_error().decode())
    return n


def device_info():
    cus, khz, mem = C.c_int(), C.c_int(), C.c_int64()
    name = C.create_string_buffer(256)
    capi.check(lib(), lib().kr_device_info(C.byref(cus), C.byref(khz), C.byref(mem), name, 256), "kr_device_info")
    return {"name": name.value.decode(), "cu_count": cus.value, "clock_khz": khz.value, "hbm_bytes": mem.value}


def trace(params, rays, inplace=False):
    """Raytracer<double>::run_raytrace on a host array of Ray<double> records. Returns (rays, stats dict)."""
    f32 = rays.dtype == capi.RAY_F32
    _rays_arg(rays, capi.RAY_F32 if f32 else capi.RAY_F64)
    out = rays if inplace else rays.copy()
    st = Stats()
    fn = lib().kr_trace_f32 if f32 else lib().kr_trace_f64
    capi.check(lib(), fn(C.byref(params), _ptr(out), len(out), C.byref(st)), "kr_trace")
    return out, st.as_dict()


def trace_dev(params, d_ptr, n, stream=None, want_stats=True, f32=False):
    st = Stats() if want_stats else None
    fn = lib().kr_trace_dev_f32 if f32 else lib().kr_trace_dev_f64
    capi.check(lib(), fn(C.byref(params), C.c_void_p(d_ptr), n, C.c_void_p(stream or 0), C.byref(st) if st else None), "kr_trace_dev")
    return st.as_dict() if st else None


def trace_async(params, d_ptr, n, stream=None, f32=False):
    """kr_trace_async_*: enqueues the trace on `stream`, returns a ticket for trace_wait / trace_release."""
    ticket = C.c_void_p()
    fn = lib().kr_trace_async_f32 if f32 else lib().kr_trace_async_f64
    capi.check(lib(), fn(C.byref(params), C.c_void_p(d_ptr), n, C.c_void_p(stream or 0), C.byref(ticket)), "kr_trace_async")
    return ticket


def trace_batch_async(params_list, d_ptrs, ns, streams=None):
    """kr_trace_batch_async_f64: all strict side launches first, then all main launches.  Returns one ticket per trace."""
    count = len(params_list)
    pp = (C.POINTER(Params) * count)(*[C.pointer(p) for p in params_list])
    dd = (C.c_void_p * count)(*[C.c_void_p(d) for d in d_ptrs])
    nn = (C.c_int64 * count)(*ns)
    ss = (C.c_void_p * count)(*[C.c_void_p(s or 0) for s in (streams or [0] * count)])
    tt = (C.c_void_p * count)()
    capi.check(lib(), lib().kr_trace_batch_async_f64(count, pp, dd, nn, ss, tt), "kr_trace_batch_async")
    return [C.c_void_p(t) for t in tt]


def trace_wait(ticket, want_stats=True):
    st = Stats() if want_stats else None
    capi.check(lib(), lib().kr_trace_wait(ticket, C.byref(st) if st else None), "kr_trace_wait")
    return st.as_dict() if st else None


def trace_wait_many(tickets):
    """kr_trace_wait_many: waits for and releases all tickets in one call; returns the summed counters (kernel_ms etc.: the largest)."""
    count = len(tickets)
    tt = (C.c_void_p * count)(*[t.value if isinstance(t, C.c_void_p) else t for t in tickets])
    tot = Stats()
    capi.check(lib(), lib().kr_trace_wait_many(count, tt, None, C.byref(tot)), "kr_trace_wait_many")
    return tot.as_dict()


def trace_release(ticket):
    capi.check(lib(), lib().kr_trace_release(ticket), "kr_trace_release")


def _pass(name, rays):
    """The f64 or f32 entry point of an O(N) pass, by the dtype of `rays`."""
    f32 = isinstance(rays, np.ndarray) and rays.dtype == capi.RAY_F32
    _rays_arg(rays, capi.RAY_F32 if f32 else capi.RAY_F64)
    return getattr(lib(), f"{name}_{'f32' if f32 else 'f64'}")


def redshift_start(spin, V, reverse, projradius, rays):
    capi.check(lib(), _pass("kr_redshift_start", rays)(spin, V, int(reverse), int(projradius), _ptr(rays), len(rays)), "kr_redshift_start")
    return rays


def redshift(spin, V, reverse, projradius, rays, motion=0):
    capi.check(lib(), _pass("kr_redshift", rays)(spin, V, int(reverse), int(projradius), motion, _ptr(rays), len(rays)), "kr_redshift")
    return rays


def redshift_dest(spin, reverse, rays):
    capi.check(lib(), _pass("kr_redshift_dest", rays)(spin, int(reverse), _ptr(rays), len(rays)), "kr_redshift_dest")
    return rays


def range_phi(rays, lo=-np.pi, hi=np.pi):
    capi.check(lib(), _pass("kr_range_phi", rays)(lo, hi, _ptr(rays), len(rays)), "kr_range_phi")
    return rays


def calculate_momentum(spin, rays):
    capi.check(lib(), _pass("kr_calculate_momentum", rays)(spin, _ptr(rays), len(rays)), "kr_calculate_momentum")
    return rays


def pointsource_count(spec):
    nc, nb = C.c_int32(), C.c_int32()
    n = lib().kr_pointsource_count(C.byref(spec), C.byref(nc), C.byref(nb))
    return n, nc.value, nb.value


def imageplane_count(spec):
    nx, ny = C.c_int32(), C.c_int32()
    n = lib().kr_imageplane_count(C.byref(spec), C.byref(nx), C.byref(ny))
    return n, nx.value, ny.value


def pointsource_init(spec):
    n, _, _ = pointsource_count(spec)
    rays = np.zeros(n, dtype=capi.RAY_F64)
    capi.check(lib(), lib().kr_pointsource_init_f64(C.byref(spec), _ptr(rays), n), "kr_pointsource_init")
    return rays


def imageplane_init(spec):
    n, _, _ = imageplane_count(spec)
    rays = np.zeros(n, dtype=capi.RAY_F64)
    capi.check(lib(), lib().kr_imageplane_init_f64(C.byref(spec), _ptr(rays), n), "kr_imageplane_init")
    return rays


def _rounded(word):
    return int(round(float(word)))


def _layout(planes, tallies, words=None):
    """The one description of a result buffer: the planes [(name, shape), ..] one after the other, then one word per tally [(name, cast), ..] (name
    None: a word without a name).  Without `words`: the buffer's length.  With words -- one buffer, or a stack of them along the leading axes -- the
    dict: every plane a copy shaped leading axes + shape, every named tally cast(its word)."""
    if words is None:
        return sum(math.prod(shape) for _, shape in planes) + len(tallies)
    words = np.asarray(words, dtype=np.float64)
    lead, out, at = words.shape[:-1], {}, 0
    for name, shape in planes:
        size = math.prod(shape)
        out[name] = words[..., at:at + size].reshape(lead + shape).copy()
        at += size
    out.update({name: cast(words[..., at + q]) for q, (name, cast) in enumerate(tallies) if name is not None})
    return out


def _emissivity_layout(bins, words=None):
    return _layout([(k, (bins.nr,)) for k in ("count", "flux", "emis", "sum_redshift", "sum_time")], [("disc_count", int)], words)


def emissivity_words(bins):
    """Length of the radial histogram buffer of kr_reduce_emissivity_dev_f64 / kr_post_emissivity_*_dev_f64: five planes of nr and disc_count."""
    return _emissivity_layout(bins)


def emissivity_from_words(bins, words):
    """The radial histogram buffer as the dict reduce_emissivity() returns (raw sums; count as int64)."""
    out = _emissivity_layout(bins, words)
    out["count"] = out["count"].astype(np.int64)
    return out


def reduce_emissivity(bins, rays):
    _rays_arg(rays, capi.RAY_F64)
    nr = bins.nr
    count = np.zeros(nr, dtype=np.int64)
    flux, emis, sg, stt = (np.zeros(nr) for _ in range(4))
    dc = C.c_int64()
    capi.check(lib(), lib().kr_reduce_emissivity_f64(C.byref(bins), _ptr(rays), len(rays), _ptr(count), _ptr(flux), _ptr(emis),
                                                     _ptr(sg), _ptr(stt), C.byref(dc)), "kr_reduce_emissivity")
    return {"count": count, "flux": flux, "emis": emis, "sum_redshift": sg, "sum_time": stt, "disc_count": dc.value}


def reduce_image(bins, rays):
    _rays_arg(rays, capi.RAY_F64)
    npix = bins.img_nx * bins.img_ny
    nrays = np.zeros(npix, dtype=np.int32)
    planes = {k: np.zeros(npix) for k in ("flux", "r", "phi", "enshift", "time", "emis")}
    dc = C.c_int64()
    capi.check(lib(), lib().kr_reduce_image_f64(C.byref(bins), _ptr(rays), len(rays), _ptr(nrays), *[_ptr(planes[k]) for k in
                                                ("flux", "r", "phi", "enshift", "time", "emis")], C.byref(dc)), "kr_reduce_image")
    out = {"nrays": nrays, "disc_count": dc.value}
    out.update(planes)
    return out


def _image_layout(nx, ny, words=None):
    return _layout([(k, (nx * ny,)) for k in ("nrays", "flux", "r", "phi", "enshift", "time", "emis")], [("disc_count", _rounded)], words)


def image_words(bins):
    """Length of the image buffer of kr_reduce_image_dev_f64 / kr_post_image_dev_f64: seven planes of img_nx img_ny and disc_count."""
    return _image_layout(bins.img_nx, bins.img_ny)


def image_planes_from_words(words, nx, ny):
    """The device-resident reducers' result buffer (kr_reduce_image_dev_f64 / kr_post_image_dev_f64: 7 nx ny + 1 doubles,
    [nrays | flux | r | phi | enshift | time | emis | disc_count]) as the dict reduce_image() returns."""
    out = _image_layout(nx, ny, words)
    return {"nrays": np.rint(out.pop("nrays")).astype(np.int32), "disc_count": out.pop("disc_count"), **out}


# ---- a disc of finite thickness (KR_STOP_THICKDISC) and the reducers for rays that landed on a surface (include/kr_trace.h) ----
def thick_disc_params(p, r_in, r_out, slope, scale):
    """A copy of the trace parameters `p` that stops on the body |z| <= H(rho), r_in <= rho <= r_out (r_out <= 0: open) of KR_STOP_THICKDISC."""
    return capi.copy_params(p, stop_kind=capi.STOP_THICKDISC, stop_params=(float(r_in), float(r_out), float(slope), float(scale)))


def surface_height(rho, r_in, slope, scale):
    """H(rho) = slope rho + scale (1 - sqrt(r_in / rho)), the half-thickness of KR_STOP_THICKDISC at the cylindrical radius rho (host numpy)."""
    rho = np.asarray(rho, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return slope * rho + scale * (1 - np.sqrt(r_in / rho))


def surface_area_density(rho, r_in, slope, scale, spin):
    """Proper area of the surface z = H(rho) per unit rho and phi for the gas on circular orbits at the cylindrical radius, Omega = 1 / (a + rho
    sqrt(rho)) -- surface_area_density of host/include/disc.h (INTEGRATION.md 3m has the formula), host numpy.  With the tangent along the surface
    T = (0, (rho + H H') / r, (H - rho H') / r^2, 0) at r = sqrt(rho^2 + H^2), theta = atan2(rho, H):
        sqrt((Sigma / Delta) T_r^2 + Sigma T_theta^2) sqrt(e2psi) / sqrt(1 - (Omega - omega)^2 e2psi / e2nu)."""
    rho = np.asarray(rho, dtype=np.float64)
    a = float(spin)
    with np.errstate(all="ignore"):
        root = np.sqrt(r_in / rho)
        H = slope * rho + scale * (1 - root)
        Hp = slope + (scale * 0.5 * root) / rho
        r = np.sqrt(rho * rho + H * H)
        theta = np.arctan2(rho, H)
        Tr, Tth = (rho + H * Hp) / r, (H - rho * Hp) / (r * r)
        st, ct = np.sin(theta), np.cos(theta)
        rhosq = r * r + (a * ct) * (a * ct)
        delta = r * r - 2 * r + a * a
        sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st
        e2nu, e2psi, omega = rhosq * delta / sigmasq, sigmasq * st * st / rhosq, 2 * a * r / sigmasq
        V = 1 / (a + rho * np.sqrt(rho))
        lorentz = 1 / np.sqrt(1 - (V - omega) * (V - omega) * e2psi / e2nu)
        return np.sqrt((rhosq / delta) * Tr * Tr + rhosq * Tth * Tth) * np.sqrt(e2psi) * lorentz


def surface_area(edges, r_in, slope, scale, spin, dphi=0.1, n_sub=50):
    """The proper area of each ring [edges[i], edges[i + 1]) of the surface z = H(rho) of KR_STOP_THICKDISC, per azimuthal width dphi, for the orbiting
    gas: integrate_surface_area of host/include/disc.h, which is the rule of the project's disc-area function integrate_disc_area -- n_sub - 1
    log-spaced sub-rings, each taken at its inner edge, non-positive and NaN pieces skipped, dphi = 0.1 as the emissivity programs pass it -- with
    the line element along the surface (surface_area_density).  At slope = scale = 0 it is integrate_disc_area(..., force_keplerian).  Host numpy."""
    edges = [float(e) for e in edges]
    out = np.zeros(max(len(edges) - 1, 0))
    for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        step = math.exp(math.log(hi / lo) / (n_sub - 1))
        subs, rho = [], lo
        while rho < hi:                                    # (the running product, as the C++ loop forms it)
            subs.append(rho)
            rho = rho * step
        subs = np.array(subs)
        pieces = surface_area_density(subs, r_in, slope, scale, spin) * (subs * (step - 1)) * dphi
        total = 0.0
        for piece in pieces.tolist():
            if piece > 0:
                total += piece
        out[i] = total
    return out


SURFACE_PLANES = ("count", "flux", "emis", "sum_redshift", "sum_time", "sum_z")
SURFACE_TALLIES = ("disc_count", "binned", "upper", "lower")


def _emissivity_surface_layout(bins, words=None):
    return _layout([(k, (bins.nr,)) for k in SURFACE_PLANES], [(k, _rounded) for k in SURFACE_TALLIES], words)


def emissivity_surface_words(bins):
    """Length of the buffer of kr_reduce_emissivity_surface_dev_f64 / kr_post_emissivity_surface_dev_f64: six planes of nr and four tallies."""
    return _emissivity_surface_layout(bins)


def emissivity_surface_from_words(bins, words):
    """That buffer as a dict: count (int64), flux, emis, sum_redshift, sum_time, sum_z (nr raw sums each), disc_count / binned / upper / lower."""
    out = _emissivity_surface_layout(bins, words)
    out["count"] = np.rint(out["count"]).astype(np.int64)
    return out


def surface_emissivity(pointsource_spec, params, bins, return_records=False):
    """The emissivity profile of a point source on a disc with a surface, resident on the device from start to finish: PointSource ctor +
    redshift_start (kr_pointsource_init_emit_dev_f64, the source's own V) -> trace (kr_trace_dev_f64; `params` with a RayDestination stop, e.g.
    thick_disc_params) -> range_phi + redshift for the Keplerian gas at the cylindrical radius + the histogram over rho
    (kr_post_emissivity_surface_dev_f64).  Only the histogram is read back (and, with return_records, the final records: for tests).
    Returns emissivity_surface_from_words(...) plus "stats" (the trace's kr_stats)."""
    L = lib()
    n, _, _ = pointsource_count(pointsource_spec)
    if n <= 0:
        raise KrError("surface_emissivity: empty ray grid")
    nw = emissivity_surface_words(bins)
    st = Stats()
    with DeviceScope(L) as dev:
        d_hist = dev.zeros(nw * 8) if bins.nr > 0 else C.c_void_p()          # (the pass refuses nr <= 0: no allocation of a negative size)
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(pointsource_spec), 0, 1, pointsource_spec.V, 0, 0, d_rays, n, None), "kr_pointsource_init_emit")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        capi.check(L, L.kr_post_emissivity_surface_dev_f64(pointsource_spec.spin, 0, -np.pi, np.pi, C.byref(bins), d_rays, n, d_hist, None), "kr_post_emissivity_surface")
        capi.check(L, L.kr_synchronize(None), "kr_synchronize")
        res = emissivity_surface_from_words(bins, dev.fetch(d_hist, nw))
        if return_records:
            res["records"] = dev.fetch(d_rays, n, capi.RAY_F64)
    res["stats"] = st.as_dict()
    return res


def surface_image(imageplane_spec, params, image_bins, return_records=False):
    """The image of a disc with a surface, resident on the device from start to finish: ImagePlane ctor + redshift_start
    (kr_imageplane_init_emit_dev_f64) -> trace (kr_trace_dev_f64; `params` as for the image app -- the stored, negated spin -- with a RayDestination
    stop, e.g. thick_disc_params) -> redshift for the Keplerian gas at the cylindrical radius + range_phi + the seven planes
    (kr_post_image_surface_dev_f64).  Only the planes are read back (and, with return_records, the final records: for tests).
    Returns image_planes_from_words(...) plus "stats" (the trace's kr_stats)."""
    L = lib()
    n, _, _ = imageplane_count(imageplane_spec)
    if n <= 0:
        raise KrError("surface_image: empty ray grid")
    sized = image_bins.img_nx > 0 and image_bins.img_ny > 0
    nw = image_words(image_bins) if sized else 0
    spin = -1 * imageplane_spec.spin                     # as stored by the Raytracer of an ImagePlane (imageplane.cpp:12)
    st = Stats()
    with DeviceScope(L) as dev:
        d_planes = dev.zeros(nw * 8) if sized else C.c_void_p()
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(imageplane_spec), 0, 1, 0.0, 1, 0, d_rays, n, None), "kr_imageplane_init_emit")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        capi.check(L, L.kr_post_image_surface_dev_f64(spin, 1, -np.pi, np.pi, C.byref(image_bins), d_rays, n, d_planes, None), "kr_post_image_surface")
        capi.check(L, L.kr_synchronize(None), "kr_synchronize")
        res = image_planes_from_words(dev.fetch(d_planes, nw), image_bins.img_nx, image_bins.img_ny)
        if return_records:
            res["records"] = dev.fetch(d_rays, n, capi.RAY_F64)
    res["stats"] = st.as_dict()
    return res


RETURN_MAP_PLANES = ("count", "weight", "flux", "emis", "time")
RETURN_MAP_SCALARS = ("ray_count", "return", "escape", "lost", "on_disc", "binned")


def _return_map_layout(nr, casts=(None,) * 6, words=None):
    return _layout([(k, (nr,)) for k in RETURN_MAP_PLANES], list(zip(RETURN_MAP_SCALARS, casts)), words)


def return_map_words(m):
    """Length of the landing-map buffer: five planes of nr and six scalars (include/kr_trace.h, kr_return_map)."""
    return _return_map_layout(m.nr)


def return_map_from_words(m, words):
    """The landing-map buffer as a dict: count / weight / flux / emis / time (nr raw sums each; count stays a double array of whole numbers),
    ray_count / return / escape / lost (weighted sums, as kr_reduce_return_f64 gives them), on_disc / binned (ints) and the nr + 1 bin edges."""
    out = _return_map_layout(m.nr, [float] * 4 + [_rounded] * 2, words)
    k = np.arange(m.nr + 1)
    out["r_edges"] = m.r_min * m.dr ** k if m.logbin else m.r_min + m.dr * k
    return out


def return_radiation_from_words(nr, words):
    """The landing-map buffers of several source radii, shaped (nsrc, return_map_words): the planes as (nsrc, nr) arrays and the six scalars as
    arrays over the radii, as return_radiation() returns them."""
    return _return_map_layout(nr, [np.copy] * 6, words)


def reduce_return_map(m, rays):
    """kr_reduce_return_map_f64: the landing map of host ray records after range_phi() and redshift(-1)."""
    _rays_arg(rays, capi.RAY_F64)
    out = np.zeros(return_map_words(m))
    capi.check(lib(), lib().kr_reduce_return_map_f64(C.byref(m), _ptr(rays), len(rays), _ptr(out)), "kr_reduce_return_map")
    return return_map_from_words(m, out)


def return_map_struct(r_isco, r_disc, r_esc, source_r, source_phi, r_min, dr, nr, logbin, gamma=2.0, plane_iso=1, limb=0, weight_norm=1):
    m = capi.ReturnMap()
    c = m.cls
    c.r_isco, c.r_disc, c.r_esc, c.source_r, c.source_phi = r_isco, r_disc, r_esc, source_r, source_phi
    c.plane_iso, c.limb, c.weight_norm, c.pad = int(plane_iso), int(limb), int(weight_norm), 0
    m.r_min, m.dr, m.gamma, m.nr, m.logbin = r_min, dr, gamma, int(nr), int(logbin)
    return m


def return_radiation_sources(spin, source_radii, dcosalpha, dbeta, source_phi=1.5707, cosalpha0=-0.995, cosalphamax=0.995):
    """The PointSources of disc_source_photonfrac_r.cpp:66-89, one per radius: on the disc (theta = pi / 2 - 1e-6), in Keplerian motion
    (V = kr_disc_velocity), beta in [0, pi)."""
    specs = []
    for r_s in source_radii:
        s = capi.PointSourceSpec()
        for i, v in enumerate((0.0, float(r_s), np.pi / 2 - 1e-6, source_phi)):
            s.pos[i] = v
        s.V, s.spin, s.tol, s.E = lib().kr_disc_velocity(float(r_s), spin, 1), spin, 100.0, 1.0
        s.cosalpha0, s.cosalphamax, s.dcosalpha = cosalpha0, cosalphamax, dcosalpha
        s.beta0, s.betamax, s.dbeta = 0.0, np.pi, dbeta
        specs.append(s)
    return specs


def _add_stats(total, st):
    for k, v in st.items():
        total[k] = v if k not in total else max(total[k], v) if k.startswith("longest_") else total[k] + v
    return total


def return_radiation(spin, source_radii, dcosalpha, dbeta, r_disc=500.0, r_esc=1000.0, r_min=None, nr=100, logbin=False, gamma=2.0, plane_iso=1, limb=0,
                     weight_norm=1, source_phi=1.5707, integrator=capi.EULER, flags=0, cosalpha0=-0.995, cosalphamax=0.995, return_records=False):
    """The disc -> disc returning-radiation sweep with its landing map, resident on the device from start to finish, as the kr_return_radiation
    app runs it: for every source radius a PointSource on the disc + redshift_start (kr_pointsource_init_emit_batch_dev_f64) -> the merged batch
    trace to theta = pi / 2 or r = 1.1 r_esc (kr_trace_batch_async_f64) -> range_phi + redshift(-1) + classification + landing map
    (kr_post_return_map_batch_dev_f64).  The landing bins are nr bins from r_min (default: the ISCO) to r_disc, linear or logarithmic.  Radii are
    processed in groups whose ray buffers stay under a quarter of the device's memory; only the (5 nr + 6)-word results are read back (and, with
    return_records, the final records: a list of arrays, for tests).
    Returns the planes count / weight / flux / emis / time as (len(source_radii), nr) arrays, the six scalars as arrays over the radii, "stats" (the
    trace counters summed over the groups), "r_isco", "r_min", "dr", "r_edges"."""
    L = lib()
    radii = [float(r) for r in source_radii]
    r_isco = L.kr_kerr_isco(spin, 1)
    r_min = r_isco if r_min is None or r_min < 0 else float(r_min)
    if nr <= 0:
        raise KrError("return_radiation: nr must be positive")
    dr = math.exp(math.log(r_disc / r_min) / nr) if logbin else (r_disc - r_min) / nr       # the C library's, as the app computes it
    specs = return_radiation_sources(spin, radii, dcosalpha, dbeta, source_phi, cosalpha0, cosalphamax)
    counts = [pointsource_count(s)[0] for s in specs]
    if any(c <= 0 for c in counts):
        raise KrError("return_radiation: empty ray grid")
    maps = [return_map_struct(r_isco, r_disc, r_esc, r_s, source_phi, r_min, dr, nr, logbin, gamma, plane_iso, limb, weight_norm) for r_s in radii]
    p = capi.default_params(spin)
    p.integrator, p.theta_max, p.r_max, p.stop_kind, p.flags = integrator, np.pi / 2, 1.1 * r_esc, capi.STOP_THETA, flags
    nsrc, nw = len(radii), _return_map_layout(nr)
    words = np.zeros((nsrc, nw))
    stats, records = {}, []
    if nsrc == 0:
        per_group = 1
    else:
        slot = (max(counts) * capi.RAY_F64.itemsize + 255) // 256 * 256
        per_group = int(max(1, min(256, (device_info()["hbm_bytes"] // 4) // slot)))
    with DeviceScope(L) as dev:
        if nsrc:
            d_out = dev.zeros(words.nbytes)
            d_rays = dev.alloc(min(per_group, nsrc) * slot)         # one slab, reused by every group
        for first in range(0, nsrc, per_group):
            idx = range(first, min(first + per_group, nsrc))
            k = len(idx)
            ss = (capi.PointSourceSpec * k)(*[specs[j] for j in idx])
            V = (C.c_double * k)(*[specs[j].V for j in idx])
            ptr_values = [d_rays.value + q * slot for q in range(k)]
            ptrs = (C.c_void_p * k)(*ptr_values)
            ns = (C.c_int64 * k)(*[counts[j] for j in idx])
            mm = (capi.ReturnMap * k)(*[maps[j] for j in idx])
            outs = (C.c_void_p * k)(*[d_out.value + 8 * nw * j for j in idx])
            capi.check(L, L.kr_pointsource_init_emit_batch_dev_f64(k, ss, V, 0, 0, ptrs, ns, None), "kr_pointsource_init_emit_batch")
            tickets = trace_batch_async([p] * k, ptr_values, [counts[j] for j in idx])
            rc = L.kr_post_return_map_batch_dev_f64(k, spin, -1.0, 0, 0, 0, -np.pi, np.pi, mm, ptrs, ns, outs, None)
            _add_stats(stats, trace_wait_many(tickets))          # the tickets are retired whatever the pass said
            capi.check(L, rc, "kr_post_return_map_batch")
            capi.check(L, L.kr_synchronize(None), "kr_synchronize")
            if return_records:
                records += [dev.fetch(C.c_void_p(ptr_values[q]), counts[j], capi.RAY_F64) for q, j in enumerate(idx)]
        if nsrc:
            dev.fetch_into(d_out, words)
    res = return_radiation_from_words(nr, words)
    e = np.arange(nr + 1)
    res.update(stats=stats, r_isco=r_isco, r_min=r_min, dr=dr, r_edges=r_min * dr ** e if logbin else r_min + dr * e, maps=maps, specs=specs)
    if return_records:
        res["records"] = records
    return res


def _line_layout(bins, words=None):
    return _layout([("count", (bins.nt, bins.ne)), ("flux", (bins.nt, bins.ne))], [("on_disc", _rounded), ("binned", _rounded)], words)


def line_words(bins):
    """Length of the line histogram buffer: [count (nt x ne) | flux (nt x ne) | on_disc | binned] (include/kr_trace.h, kr_line_bins)."""
    return _line_layout(bins)


def line_from_words(bins, words):
    """The histogram buffer of the line entry points as a dict: count / flux of shape (nt, ne), on_disc, binned, and the bin edges
    (time_edges is None without a time axis)."""
    out = _line_layout(bins, words)
    k = np.arange(bins.ne + 1)
    out["energy_edges"] = bins.e_min * bins.de ** k if bins.log_e else bins.e_min + bins.de * k
    out["time_edges"] = None if (bins.nt == 1 and bins.dt <= 0) else bins.t0 + bins.dt * np.arange(bins.nt + 1)
    return out


def reduce_line(bins, rays):
    """kr_reduce_line_f64: the emission line (or transfer function) of host ray records after redshift(-1, reverse=1)."""
    _rays_arg(rays, capi.RAY_F64)
    out = np.zeros(line_words(bins))
    capi.check(lib(), lib().kr_reduce_line_f64(C.byref(bins), _ptr(rays), len(rays), _ptr(out)), "kr_reduce_line")
    return line_from_words(bins, out)


def default_image_bins(spec, bins):
    """One pixel per ray of the image plane `spec`, centred on it (img_dx = dx, the grid shifted by half a pixel, so no ray sits on a pixel
    edge or off the grid), with the disc filter and powerlaw3 of the line bins."""
    _, nx, ny = imageplane_count(spec)
    ib = capi.ImageBins()
    ib.x0, ib.y0, ib.img_dx, ib.img_dy = spec.x0 - spec.dx / 2, spec.y0 - spec.dy / 2, spec.dx, spec.dy
    ib.r_isco, ib.r_disc = bins.r_isco, bins.r_disc
    ib.q1, ib.rb1, ib.q2, ib.rb2, ib.q3 = bins.q1, bins.rb1, bins.q2, bins.rb2, bins.q3
    ib.img_nx, ib.img_ny, ib.flip_image = nx, ny, 1
    return ib


def _surface_arg(what, surface, V=-1.0, pol=None):
    """The capi.DiscSurface of a surface= argument; the surface passes keep the Keplerian observer at rho and carry no polarisation."""
    if V == capi.V_PLUNGE:
        raise KrError(f"{what}: surface cannot be combined with V = V_PLUNGE (the surface passes keep the Keplerian observer at rho)")
    if pol is not None:
        raise KrError(f"{what}: surface cannot be combined with pol (the Stokes passes know no surface)")
    return capi.disc_surface(surface)


def _illum_arg(what, illum, V=-1.0, surface=None, pol=None):
    """The capi.IllumTable of an illum= argument (an IllumTable, or the dict of illumination_table); the table passes are flat, unpolarised and Keplerian."""
    if surface is not None or pol is not None or V == capi.V_PLUNGE:
        raise KrError(f"{what}: illum cannot be combined with surface, pol or V = V_PLUNGE (the table passes are the flat, unpolarised, Keplerian ones)")
    return illum if isinstance(illum, capi.IllumTable) else capi.illum_table(illum)


def line_profile(imageplane_spec, params, bins, mode="rays", image_bins=None, limb=None, V=-1.0, surface=None, illum=None):
    """The emission line of an image plane, resident on the device from start to finish, as the kr_line_profile app runs it:
    ImagePlane ctor + redshift_start (kr_imageplane_init_emit_dev_f64) -> trace (kr_trace_dev_f64) -> either
      mode="rays":   redshift + range_phi + line bins per ray (kr_post_line_dev_f64), or
      mode="pixels": redshift + range_phi + the image planes (kr_post_image_dev_f64, `image_bins`; default: one pixel per ray)
                     -> line bins per pixel, the notebook's form (kr_line_from_image_dev_f64).
    `params` as for the image app: the stored (negated) spin, theta / r limits, integrator.  Only the histogram is read back.
    limb (mode="rays" only): None for the isotropic line through kr_post_line_dev_f64, or a limb law of the emission angle in the disc frame --
    (law, coeff) or "isotropic", "laor" (1 + 2.06 mu), "brightening" (log(1 + 1 / mu)) -- through kr_post_line_limb_dev_f64.
    V: the disc flow of the redshift, -1 Keplerian or capi.V_PLUNGE (plunging inside the ISCO: set bins.r_isco to the inner radius wanted).
    surface (mode="rays" only): None, or the surface of a disc of finite thickness -- (r_in, r_out, slope, scale) or a capi.DiscSurface; trace to it with
    thick_disc_params(...), as for surface_image.  The line is then that of the rays that LANDED on the surface, binned by rho = r sin(theta), the
    emission angle taken to the surface normal (kr_post_line_surface_dev_f64; limb None is the isotropic law) and "bad_angle" is always there.
    V = capi.V_PLUNGE is refused with a surface.
    illum (mode="rays" only): None, or an (r, phi) illumination table -- a capi.IllumTable or the dict of illumination_table -- that gives every disc cell
    its emissivity and source -> disc delay in place of powerlaw3 / the bins' radial table (kr_post_line_illum_dev_f64; limb None is the isotropic law,
    and "bad_angle" is always there).  Its phi_shift is the orbital phase of the source (capi.illum_table).  Refused with surface or V = capi.V_PLUNGE.
    With illum=None the calls are exactly those made without the argument.
    Returns line_from_words(...) plus "stats" (the trace's kr_stats) and, with a limb law, "bad_angle"."""
    if illum is not None:
        table = _illum_arg("line_profile", illum, V, surface)
        if mode != "rays":
            raise KrError("line_profile: illum needs mode='rays'")
        law = capi.limb_law(limb if limb is not None else "isotropic")
        words, stats, _ = _imageplane_run("line_profile", imageplane_spec, params, line_words(bins) + 1, lambda L, dev, d_rays, n, d_out: capi.check(
            L, L.kr_post_line_illum_dev_f64(-1 * imageplane_spec.spin, V, 1, 0, 0, -np.pi, np.pi, C.byref(bins), C.byref(law), C.byref(table), d_rays, n, d_out, None),
            "kr_post_line_illum"))
        res = line_from_words(bins, words[:-1])
        res["stats"], res["bad_angle"] = stats, _rounded(words[-1])
        return res
    if surface is not None:
        sf = _surface_arg("line_profile", surface, V)
        if mode != "rays":
            raise KrError("line_profile: a surface needs mode='rays'")
        law = capi.limb_law(limb if limb is not None else "isotropic")
        words, stats, _ = _imageplane_run("line_profile", imageplane_spec, params, line_words(bins) + 1, lambda L, dev, d_rays, n, d_out: capi.check(
            L, L.kr_post_line_surface_dev_f64(C.byref(sf), -1 * imageplane_spec.spin, 1, -np.pi, np.pi, C.byref(bins), C.byref(law), d_rays, n, d_out, None),
            "kr_post_line_surface"))
        res = line_from_words(bins, words[:-1])
        res["stats"], res["bad_angle"], res["surface"] = stats, _rounded(words[-1]), (sf.r_in, sf.r_out, sf.slope, sf.scale)
        return res
    if mode not in ("rays", "pixels"):
        raise KrError(f"line_profile: mode must be 'rays' or 'pixels', got {mode!r}")
    if limb is not None and mode != "rays":
        raise KrError("line_profile: a limb law needs mode='rays' (a pixel's mean has no emission angle)")
    law = capi.limb_law(limb) if limb is not None else None
    L = lib()
    n, _, _ = imageplane_count(imageplane_spec)
    if n <= 0:
        raise KrError("line_profile: empty ray grid")
    spin = -1 * imageplane_spec.spin                     # as stored by the Raytracer of an ImagePlane (imageplane.cpp:12)
    nw = line_words(bins) + (1 if law is not None else 0)
    st = Stats()
    with DeviceScope(L) as dev:
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        d_line = dev.zeros(nw * 8)
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(imageplane_spec), 0, 1, 0.0, 1, 0, d_rays, n, None), "kr_imageplane_init_emit")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        if law is not None:
            capi.check(L, L.kr_post_line_limb_dev_f64(spin, V, 1, 0, 0, -np.pi, np.pi, C.byref(bins), C.byref(law), d_rays, n, d_line, None), "kr_post_line_limb")
        elif mode == "rays":
            capi.check(L, L.kr_post_line_dev_f64(spin, V, 1, 0, 0, -np.pi, np.pi, C.byref(bins), d_rays, n, d_line, None), "kr_post_line")
        else:
            ib = image_bins if image_bins is not None else default_image_bins(imageplane_spec, bins)
            d_planes = dev.zeros(image_words(ib) * 8)
            capi.check(L, L.kr_post_image_dev_f64(spin, V, 1, 0, 0, -np.pi, np.pi, C.byref(ib), d_rays, n, d_planes, None), "kr_post_image")
            capi.check(L, L.kr_line_from_image_dev_f64(C.byref(bins), C.byref(ib), d_planes, d_line, None), "kr_line_from_image")
        out = dev.fetch(d_line, nw)
    res = line_from_words(bins, out)
    res["stats"] = st.as_dict()
    if law is not None:
        res["bad_angle"] = _rounded(out[-1])
    return res


def arrival_angles(rays, spin, V=-1.0, reverse=0, projradius=0, surface=None):
    """kr_angles_f64 / kr_angles_dev_f64: (mu, chi) of every record in the rest frame of the orbiting gas, the observer of redshift(spin, V, reverse,
    projradius).  mu = |P_th| / E is the cosine of the angle to the disc normal, chi = atan2(P_phi, P_r) the azimuth about it; NaN for records with
    steps <= 0; a bad-angle record (mu not finite or > 1: include/kr_trace.h) keeps its values.  rays: a host array of Ray<double> records, or
    (device pointer, n) for records that are already on the device.
    surface: None, or (r_in, r_out, slope, scale) / a capi.DiscSurface: the angles to the normal of that surface in the frame of the Keplerian gas at
    rho = r sin(theta) (kr_angles_surface_f64 / kr_angles_surface_dev_f64: mu = |P_n| / E, chi = atan2(P_phi, P_s)); V and projradius are then not read
    (V = capi.V_PLUNGE is refused)."""
    L = lib()
    sf = _surface_arg("arrival_angles", surface, V) if surface is not None else None
    if isinstance(rays, tuple):
        d_ptr, n = rays
        d = d_ptr if isinstance(d_ptr, C.c_void_p) else C.c_void_p(d_ptr)
        with DeviceScope(L) as dev:
            d_out = dev.alloc(2 * n * 8) if n > 0 else C.c_void_p()
            if sf is not None:
                capi.check(L, L.kr_angles_surface_dev_f64(C.byref(sf), spin, int(reverse), d, n, d_out, None), "kr_angles_surface_dev")
            else:
                capi.check(L, L.kr_angles_dev_f64(spin, V, int(reverse), int(projradius), 0, d, n, d_out, None), "kr_angles_dev")
            out = dev.fetch(d_out, 2 * n)
    else:
        _rays_arg(rays, capi.RAY_F64)
        out = np.zeros(2 * len(rays))
        if sf is not None:
            capi.check(L, L.kr_angles_surface_f64(C.byref(sf), spin, int(reverse), _ptr(rays), len(rays), _ptr(out)), "kr_angles_surface")
        else:
            capi.check(L, L.kr_angles_f64(spin, V, int(reverse), int(projradius), 0, _ptr(rays), len(rays), _ptr(out)), "kr_angles")
    return out[0::2].copy(), out[1::2].copy()


def _emissivity_mu_layout(bins, nmu, words=None):
    return _layout([("count2", (bins.nr, nmu)), ("flux2", (bins.nr, nmu)), ("sum_mu", (bins.nr,))], [(k, int) for k in ("disc_count", "binned", "bad_angle")], words)


def emissivity_mu_words(bins, nmu):
    """Length of the by-angle buffer of kr_post_emissivity_mu_dev_f64: [count2 (nr x nmu) | flux2 (nr x nmu) | sum_mu (nr) | disc_count, binned, bad_angle]."""
    return _emissivity_mu_layout(bins, nmu)


def emissivity_mu_from_words(bins, nmu, words):
    """The by-angle buffer as a dict: count2 (int64) and flux2 of shape (nr, nmu), sum_mu (nr) and the tallies disc_count / binned / bad_angle."""
    out = _emissivity_mu_layout(bins, nmu, words)
    out["count2"] = out["count2"].astype(np.int64)
    return out


def emissivity_angles(pointsource_spec, params, bins, nmu, V=-1.0, reverse=0, projradius=0):
    """The emissivity of a point source split by incidence angle, resident on the device from start to finish, as the kr_emissivity app runs it:
    PointSource ctor + redshift_start (kr_pointsource_init_emit_dev_f64, the source's own V) -> trace (kr_trace_dev_f64) -> range_phi + redshift(V) +
    the radial histogram + its split by mu (kr_post_emissivity_mu_dev_f64).  Only the two histograms are read back.
    Returns (hist, count2, flux2, mean_mu, tallies): hist as reduce_emissivity returns it (raw sums); count2 (int64) and flux2 of shape (nr, nmu);
    mean_mu per radial bin over the rays of count2 (NaN where there are none); tallies = {"disc_count", "binned", "bad_angle", "stats"}."""
    L = lib()
    n, _, _ = pointsource_count(pointsource_spec)
    if n <= 0:
        raise KrError("emissivity_angles: empty ray grid")
    nh, nm = emissivity_words(bins), emissivity_mu_words(bins, nmu)
    mb = capi.MuBins(int(nmu), 0)
    st = Stats()
    with DeviceScope(L) as dev:
        sized = bins.nr > 0 and nmu >= 1           # (the pass below refuses the rest: it gets null buffers, no allocation of a negative size)
        d_hist = dev.zeros(nh * 8) if sized else C.c_void_p()
        d_mu = dev.zeros(nm * 8) if sized else C.c_void_p()
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(pointsource_spec), 0, 1, pointsource_spec.V, int(reverse), int(projradius), d_rays, n, None),
                   "kr_pointsource_init_emit")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        capi.check(L, L.kr_post_emissivity_mu_dev_f64(pointsource_spec.spin, V, int(reverse), int(projradius), 0, -np.pi, np.pi, C.byref(bins), C.byref(mb), d_rays, n,
                                                      d_hist, d_mu, None), "kr_post_emissivity_mu")
        hist = emissivity_from_words(bins, dev.fetch(d_hist, nh))
        by_mu = emissivity_mu_from_words(bins, nmu, dev.fetch(d_mu, nm))
    count2, flux2, sum_mu = (by_mu.pop(k) for k in ("count2", "flux2", "sum_mu"))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_mu = sum_mu / count2.sum(axis=1)
    return hist, count2, flux2, mean_mu, {**by_mu, "stats": st.as_dict()}


# ---- polarisation of disc emission on an image plane (include/kr_trace.h, kr_pol_law) ----
def polarisation(rays, spin, inc_deg, V=-1.0, projradius=0):
    """kr_polarisation_f64 / kr_polarisation_dev_f64: the Walker-Penrose constant and the polarisation angle at the observer of every record of an
    image plane seen at inclination inc_deg, for emission polarised in the disc plane perpendicular to the projected photon direction, in the rest
    frame of the orbiting gas (the observer of redshift(spin, V, reverse = 1, projradius)).  Returns {"kappa1", "kappa2", "c2", "s2"}: c2, s2 = cos, sin
    of twice the angle, from the image's x axis towards its y axis; NaN for records with steps <= 0; a bad-pol record (include/kr_trace.h) keeps its
    values.  rays: a host array of Ray<double> records, or (device pointer, n) for records that are already on the device."""
    L = lib()
    if isinstance(rays, tuple):
        d_ptr, n = rays
        d = d_ptr if isinstance(d_ptr, C.c_void_p) else C.c_void_p(d_ptr)
        with DeviceScope(L) as dev:
            d_out = dev.alloc(4 * n * 8) if n > 0 else C.c_void_p()
            capi.check(L, L.kr_polarisation_dev_f64(spin, V, 1, int(projradius), 0, inc_deg, d, n, d_out, None), "kr_polarisation_dev")
            out = dev.fetch(d_out, 4 * n)
    else:
        _rays_arg(rays, capi.RAY_F64)
        out = np.zeros(4 * len(rays))
        capi.check(L, L.kr_polarisation_f64(spin, V, 1, int(projradius), 0, inc_deg, _ptr(rays), len(rays), _ptr(out)), "kr_polarisation")
    return {k: out[q::4].copy() for q, k in enumerate(("kappa1", "kappa2", "c2", "s2"))}


def _degree_and_angle(out):
    """pdeg = sqrt(Q^2 + U^2) / I (NaN where I == 0) and evpa = atan2(U, Q) / 2 of a dict with I, Q, U; returns it."""
    with np.errstate(invalid="ignore", divide="ignore"):
        out["pdeg"] = np.where(out["I"] == 0, np.nan, np.hypot(out["Q"], out["U"]) / out["I"])
    out["evpa"] = 0.5 * np.arctan2(out["U"], out["Q"])
    return out


def _stokes_image_layout(nx, ny, words=None):
    return _layout([(k, (nx * ny,)) for k in ("nrays", "I", "Q", "U")], [("disc_count", _rounded), ("bad_pol", _rounded)], words)


def stokes_image_words(bins):
    """Length of the buffer of kr_post_image_stokes_dev_f64: four planes of img_nx img_ny, disc_count and bad_pol."""
    return _stokes_image_layout(bins.img_nx, bins.img_ny)


def stokes_image_from_words(bins, words):
    """The buffer of kr_post_image_stokes_dev_f64 as a dict: nrays (int32), I, Q, U (raw sums, [ix img_ny + iy]), disc_count, bad_pol, and per pixel
    pdeg and evpa (radians, from the image's x axis towards its y axis)."""
    out = _stokes_image_layout(bins.img_nx, bins.img_ny, words)
    out["nrays"] = np.rint(out["nrays"]).astype(np.int32)
    return _degree_and_angle(out)


def _stokes_line_layout(bins, words=None):
    return _layout([(k, (bins.nt, bins.ne)) for k in ("count", "I", "Q", "U")], [(k, _rounded) for k in ("on_disc", "binned", "bad_pol")], words)


def stokes_line_words(bins):
    """Length of the buffer of kr_post_line_stokes_dev_f64: [count | I | Q | U] (nt x ne each) + on_disc, binned, bad_pol."""
    return _stokes_line_layout(bins)


def stokes_line_from_words(bins, words):
    """The buffer of kr_post_line_stokes_dev_f64 as a dict: count, I, Q, U of shape (nt, ne), on_disc, binned, bad_pol, pdeg, evpa and the bin edges of
    line_from_words."""
    out = _degree_and_angle(_stokes_line_layout(bins, words))
    edges = line_from_words(bins, np.zeros(line_words(bins)))
    out["energy_edges"], out["time_edges"] = edges["energy_edges"], edges["time_edges"]
    return out


def _imageplane_run(what, imageplane_spec, params, nw, post, return_records=False, before=None):
    """ImagePlane ctor + redshift_start -> trace -> post(L, dev, d_rays, n, d_out), one pass or several into the nw zeroed words of d_out (nw == 0: a
    null buffer, for sizes the pass refuses): (the words, stats, records or None).  before(L, dev) runs inside the scope before anything is traced."""
    L = lib()
    n, _, _ = imageplane_count(imageplane_spec)
    if n <= 0:
        raise KrError(f"{what}: empty ray grid")
    st = Stats()
    with DeviceScope(L) as dev:
        if before is not None:
            before(L, dev)
        d_out = dev.zeros(nw * 8) if nw > 0 else C.c_void_p()
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(imageplane_spec), 0, 1, 0.0, 1, 0, d_rays, n, None), "kr_imageplane_init_emit")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        post(L, dev, d_rays, n, d_out)
        capi.check(L, L.kr_synchronize(None), "kr_synchronize")
        return dev.fetch(d_out, nw), st.as_dict(), dev.fetch(d_rays, n, capi.RAY_F64) if return_records else None


def stokes_image(imageplane_spec, params, image_bins, pol, limb=None, return_records=False):
    """The polarised image of the disc, resident on the device from start to finish: ImagePlane ctor + redshift_start
    (kr_imageplane_init_emit_dev_f64) -> trace (kr_trace_dev_f64; `params` as for the image app: the stored, negated spin) -> redshift + range_phi +
    the Stokes planes (kr_post_image_stokes_dev_f64) at the plane's own inclination.  pol: (law, coeff) or a name of capi.POL_LAWS; limb: None
    (isotropic) or a limb law as for line_profile.  Only the planes are read back (and, with return_records, the final records: for tests).
    Returns stokes_image_from_words(...) plus "stats" (the trace's kr_stats)."""
    law, plaw = capi.limb_law(limb if limb is not None else "isotropic"), capi.pol_law(pol)
    sized = image_bins.img_nx > 0 and image_bins.img_ny > 0          # (the pass refuses the rest: it gets a null buffer)
    words, stats, records = _imageplane_run("stokes_image", imageplane_spec, params, stokes_image_words(image_bins) if sized else 0, lambda L, dev, d_rays, n, d_out: capi.check(
        L, L.kr_post_image_stokes_dev_f64(-1 * imageplane_spec.spin, -1.0, 1, 0, 0, -np.pi, np.pi, imageplane_spec.inc_deg, C.byref(image_bins), C.byref(law), C.byref(plaw), d_rays, n, d_out,
                                          None), "kr_post_image_stokes"), return_records)
    res = stokes_image_from_words(image_bins, words)
    res["stats"] = stats
    if return_records:
        res["records"] = records
    return res


def stokes_line(imageplane_spec, params, line_bins, pol, limb=None):
    """The energy-resolved (and, with a time axis, time-resolved) Stokes parameters of the disc's line emission: stokes_image's pipeline with
    kr_post_line_stokes_dev_f64 as its last pass.  Returns stokes_line_from_words(...) plus "stats"."""
    law, plaw = capi.limb_law(limb if limb is not None else "isotropic"), capi.pol_law(pol)
    words, stats, _ = _imageplane_run("stokes_line", imageplane_spec, params, stokes_line_words(line_bins), lambda L, dev, d_rays, n, d_out: capi.check(
        L, L.kr_post_line_stokes_dev_f64(-1 * imageplane_spec.spin, -1.0, 1, 0, 0, -np.pi, np.pi, imageplane_spec.inc_deg, C.byref(line_bins), C.byref(law), C.byref(plaw), d_rays, n, d_out,
                                         None), "kr_post_line_stokes"))
    res = stokes_line_from_words(line_bins, words)
    res["stats"] = stats
    return res


CAUSTIC_PLANES = ("det_j", "sign_j", "order", "hit", "radius", "phi", "x_disc", "y_disc", "redshift")
CAUSTIC_COUNTS = ("disc_count", "horizon", "rlim", "steplim", "out_of_range", "other", "suppressed")


def bundles_count(spec):
    nx, ny = C.c_int32(), C.c_int32()
    n = lib().kr_bundles_count(C.byref(spec), C.byref(nx), C.byref(ny))
    return n, nx.value, ny.value


def _map_words(m, planes, counts, words=None):
    """Length of a map buffer of len(planes) planes of nx ny and len(counts) counts; with `words`, that buffer as a dict instead."""
    return _layout([(k, (m.nx, m.ny)) for k in planes], [(k, _rounded) for k in counts], words)


def caustic_words(cm):
    """Length of the map buffer of the caustic entry points: nine planes of nx ny and seven counts (include/kr_trace.h, kr_caustic_map)."""
    return _map_words(cm, CAUSTIC_PLANES, CAUSTIC_COUNTS)


def caustic_from_words(cm, words):
    """The map buffer as a dict: the nine planes as (nx, ny) arrays ([ix, iy], like Array2D) and the seven counts as ints."""
    return _map_words(cm, CAUSTIC_PLANES, CAUSTIC_COUNTS, words)


def caustic_trace_params(imageplane_spec, r_disc, integrator=capi.RK4, rk45_tol=1e-8, precision=100, flags=0, steplim=0):
    """The trace of the caustic_discplane program (caustic_discplane.cpp:167, :216): to a DiscWithISCODestination(r_isco, r_disc) -- its descriptor as
    host/raytracer/ray_destination.h::describe gives it, {r_isco, r_out, theta_lim = pi / 2, 0} -- or r_max = 1.1 dist.  Returns (params, r_isco)."""
    r_isco = lib().kr_kerr_isco(imageplane_spec.spin, 1)
    p = capi.default_params(-1 * imageplane_spec.spin)   # as stored by the Raytracer of an ImagePlane (imageplane.cpp:12)
    p.precision, p.integrator, p.flags, p.steplim = precision, integrator, flags, steplim
    if integrator == capi.RK45:
        p.rk45_tol = rk45_tol
    p.r_max = 1.1 * imageplane_spec.dist
    p.stop_kind = capi.STOP_DISC_ISCO
    for i, v in enumerate((r_isco, r_disc, np.pi / 2, 0.0)):
        p.stop_params[i] = v
    return p, r_isco


def caustic_map(imageplane_spec, r_disc, integrator=capi.RK4, eps_frac=0.01, rk45_tol=1e-8, precision=100, flags=0, steplim=0):
    """The critical-curve maps of the disc on an image plane, resident on the device from start to finish, as the kr_caustic_discplane app runs
    them: 5-ray bundles + redshift_start (kr_bundles_init_emit_dev_f64; eps_frac = 0: the plain grid, kr_imageplane_init_emit_dev_f64 and the
    grid-neighbour Jacobian) -> trace to the disc (kr_trace_dev_f64, KR_STOP_DISC_ISCO) -> redshift + maps (kr_post_caustic_disc_dev_f64) ->
    branch-boundary suppression (kr_caustic_suppress_dev_f64).  flags = 0 is the strict arithmetic (the app's default).  Only the maps are read
    back.  Returns caustic_from_words(...) plus "stats" (the trace's kr_stats), "r_isco", "eps_x", "eps_y"."""
    L = lib()
    if integrator not in (capi.RK4, capi.RK45):
        raise KrError("caustic_map: the integrator must be RK4 or RK45 (a RayDestination has no Euler form)")
    bundles = eps_frac > 0
    n, nx, ny = bundles_count(imageplane_spec) if bundles else imageplane_count(imageplane_spec)
    if n <= 0:
        raise KrError("caustic_map: empty ray grid")
    p, r_isco = caustic_trace_params(imageplane_spec, r_disc, integrator, rk45_tol, precision, flags, steplim)
    cm = capi.CausticMap()
    cm.r_isco, cm.r_disc, cm.nx, cm.ny, cm.bundles = r_isco, r_disc, nx, ny, int(bundles)
    cm.eps_x, cm.eps_y = (eps_frac * imageplane_spec.dx, eps_frac * imageplane_spec.dy) if bundles else (imageplane_spec.dx, imageplane_spec.dy)
    spin = -1 * imageplane_spec.spin
    st = Stats()
    with DeviceScope(L) as dev:
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        d_maps = dev.alloc(caustic_words(cm) * 8)
        if bundles:
            capi.check(L, L.kr_bundles_init_emit_dev_f64(C.byref(imageplane_spec), eps_frac, 0.0, 1, 0, d_rays, n, None), "kr_bundles_init_emit")
        else:
            capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(imageplane_spec), 0, 1, 0.0, 1, 0, d_rays, n, None), "kr_imageplane_init_emit")
        capi.check(L, L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        capi.check(L, L.kr_post_caustic_disc_dev_f64(spin, 1, C.byref(cm), d_rays, n, d_maps, None), "kr_post_caustic_disc")
        capi.check(L, L.kr_caustic_suppress_dev_f64(C.byref(cm), d_maps, None), "kr_caustic_suppress")
        res = caustic_from_words(cm, dev.fetch(d_maps, caustic_words(cm)))
    res.update(stats=st.as_dict(), r_isco=r_isco, eps_x=cm.eps_x, eps_y=cm.eps_y)
    return res


SOURCE_CAUSTIC_PLANES = {"sphere": ("det_j", "sign_j", "order", "escaped", "theta_s", "phi_s", "rdot_flips", "equat_cross"),
                         "plane": ("det_j", "sign_j", "order", "hit_plane", "x_s", "y_s", "rdot_flips", "equat_cross")}
SOURCE_CAUSTIC_COUNTS = {"sphere": ("escaped_count", "captured", "steplim"), "plane": ("hit_count", "captured", "steplim")}
SOURCE_KINDS = ("sphere", "plane")


def source_caustic_words(sm):
    """Length of the map buffer of kr_post_caustic_source_dev_f64: eight planes of nx ny and three counts (include/kr_trace.h, kr_source_map)."""
    kind = SOURCE_KINDS[sm.kind]
    return _map_words(sm, SOURCE_CAUSTIC_PLANES[kind], SOURCE_CAUSTIC_COUNTS[kind])


def source_caustic_from_words(sm, words):
    """The map buffer as a dict: the eight planes as (nx, ny) arrays ([ix, iy], like Array2D), named after the kind's FITS extensions, and the three
    counts as ints."""
    kind = SOURCE_KINDS[sm.kind]
    return _map_words(sm, SOURCE_CAUSTIC_PLANES[kind], SOURCE_CAUSTIC_COUNTS[kind], words)


def caustic_trace_params_source(imageplane_spec, kind, r_lim=None, z_s=None, r_max=None, integrator=capi.RK45, rk45_tol=1e-8, precision=100, flags=0, steplim=0):
    """The trace of the caustic_sourceplane program (kind "sphere", caustic_sourceplane.cpp:155: the theta-limit overload with theta_max = 0, which
    switches the equatorial stop off, to r_max = r_lim, default 1.5 dist) or of the caustic_plane program (kind "plane", caustic_plane.cpp:151, :203:
    to a FlatPlaneDestination(incl pi / 180, phi0, z_s) -- its descriptor as host/raytracer/ray_destination.h::describe gives it, {incl, phi0, z_s, 0} --
    or r_max; z_s defaults to dist, r_max to 4 z_s).  Returns (params, geometry): geometry holds r_lim, or z_s, r_max and incl_rad."""
    if kind not in SOURCE_KINDS:
        raise KrError(f"caustic_trace_params_source: kind must be one of {SOURCE_KINDS}, got {kind!r}")
    p = capi.default_params(-1 * imageplane_spec.spin)   # as stored by the Raytracer of an ImagePlane (imageplane.cpp:12)
    p.precision, p.integrator, p.flags, p.steplim = precision, integrator, flags, steplim
    if integrator == capi.RK45:
        p.rk45_tol = rk45_tol
    if kind == "sphere":
        r_lim = 1.5 * imageplane_spec.dist if r_lim is None else r_lim
        p.stop_kind, p.theta_max, p.r_max = capi.STOP_THETA, 0.0, r_lim
        return p, {"r_lim": r_lim}
    z_s = imageplane_spec.dist if z_s is None else z_s
    r_max = 4.0 * z_s if r_max is None else r_max
    incl_rad = imageplane_spec.inc_deg * np.pi / 180.0
    p.stop_kind, p.r_max = capi.STOP_FLATPLANE, r_max
    for i, v in enumerate((incl_rad, imageplane_spec.phi0, z_s, 0.0)):
        p.stop_params[i] = v
    return p, {"z_s": z_s, "r_max": r_max, "incl_rad": incl_rad}


def source_map_struct(kind, nx, ny, eps_x, eps_y, bundles=False, incl_rad=0.0, phi0=0.0):
    """kr_source_map with the four sines and cosines of a FlatPlaneDestination evaluated by the C library (math.sin / math.cos), as the reference
    evaluates them in source_coords."""
    sm = capi.SourceMap()
    sm.kind, sm.bundles, sm.nx, sm.ny, sm.eps_x, sm.eps_y = SOURCE_KINDS.index(kind), int(bundles), nx, ny, eps_x, eps_y
    sm.sin_incl, sm.cos_incl, sm.sin_phi0, sm.cos_phi0 = math.sin(incl_rad), math.cos(incl_rad), math.sin(phi0), math.cos(phi0)
    return sm


def caustic_source_map(imageplane_spec, kind, r_lim=None, z_s=None, r_max=None, integrator=capi.RK45, eps_frac=0.01, rk45_tol=1e-8, precision=100, flags=0,
                       steplim=0):
    """The caustic maps of the source sphere (kind "sphere") or of a flat source plane behind the hole (kind "plane"), resident on the device from
    start to finish, as the kr_caustic_sourceplane / kr_caustic_plane apps run them: the ray grid (kr_imageplane_init_dev_f64) or, for the plane with
    eps_frac > 0, 5-ray bundles (kr_bundles_init_emit_dev_f64) -> trace (kr_trace_dev_f64 with caustic_trace_params_source) -> gather + Jacobian
    (kr_post_caustic_source_dev_f64).  The sphere has no bundle mode: eps_frac is not read.  flags = 0 is the strict arithmetic (the apps' default).
    Only the maps are read back.  Returns source_caustic_from_words(...) plus "stats" (the trace's kr_stats), "eps_x", "eps_y" and the geometry of
    caustic_trace_params_source."""
    L = lib()
    if integrator not in (capi.RK4, capi.RK45):
        raise KrError("caustic_source_map: the integrator must be RK4 or RK45")
    p, geo = caustic_trace_params_source(imageplane_spec, kind, r_lim, z_s, r_max, integrator, rk45_tol, precision, flags, steplim)
    bundles = kind == "plane" and eps_frac > 0
    n, nx, ny = bundles_count(imageplane_spec) if bundles else imageplane_count(imageplane_spec)
    if n <= 0:
        raise KrError("caustic_source_map: empty ray grid")
    eps_x, eps_y = (eps_frac * imageplane_spec.dx, eps_frac * imageplane_spec.dy) if bundles else (imageplane_spec.dx, imageplane_spec.dy)
    sm = source_map_struct(kind, nx, ny, eps_x, eps_y, bundles, geo.get("incl_rad", 0.0), imageplane_spec.phi0)
    st = Stats()
    with DeviceScope(L) as dev:
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        d_maps = dev.alloc(source_caustic_words(sm) * 8)
        if bundles:
            capi.check(L, L.kr_bundles_init_emit_dev_f64(C.byref(imageplane_spec), eps_frac, 0.0, 1, 0, d_rays, n, None), "kr_bundles_init_emit")
        else:
            capi.check(L, L.kr_imageplane_init_dev_f64(C.byref(imageplane_spec), d_rays, n, None), "kr_imageplane_init")
        capi.check(L, L.kr_trace_dev_f64(C.byref(p), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        capi.check(L, L.kr_post_caustic_source_dev_f64(C.byref(sm), d_rays, n, d_maps, None), "kr_post_caustic_source")
        res = source_caustic_from_words(sm, dev.fetch(d_maps, source_caustic_words(sm)))
    res.update(geo, stats=st.as_dict(), eps_x=eps_x, eps_y=eps_y)
    return res


def path_spec(write_step=1, write_rmin=-1.0, write_rmax=-1.0):
    w = capi.PathSpec()
    w.write_step, w.write_rmin, w.write_rmax = int(write_step), write_rmin, write_rmax
    return w


def rows_to_cartesian(rows, spin):
    """(t, r, theta, phi) rows -> (t, x, y, z) with cartesian() of the reference (src/include/kerr.h:41-48), evaluated on the host with the C
    library's sqrt / sin / cos through the math module (numpy's vectorised sin / cos need not round like it), one row at a time."""
    out = np.empty_like(rows)
    a = float(spin)
    for i, (t, r, theta, phi) in enumerate(rows.tolist()):
        rho = math.sqrt(r * r + a * a) if r == r else r
        st, ct = (math.sin(theta), math.cos(theta)) if math.isfinite(theta) else (math.nan, math.nan)
        sp, cp = (math.sin(phi), math.cos(phi)) if math.isfinite(phi) else (math.nan, math.nan)
        out[i] = (t, rho * st * cp, rho * st * sp, r * ct)
    return out


def trace_paths(params, rays, write_step=1, write_rmin=-1.0, write_rmax=-1.0, cartesian=False, spin=None):
    """run_raytrace(..., outfile, write_step, write_rmax, write_rmin, write_cartesian) on a host array of Ray<double> records
    (kr_trace_paths_f64: Euler / RK4, strict arithmetic).  Returns (offsets, rows, traced, rays_out, stats): ray i owns
    rows[offsets[i]:offsets[i + 1]], a row is (t, r, theta, phi) -- or (t, x, y, z) with cartesian=True (spin: the Raytracer's, default
    params.spin); traced[i] == 0 for rays the skip rule left out; rays_out are the final records, as trace() gives them."""
    _rays_arg(rays, capi.RAY_F64)
    L = lib()
    out = rays.copy()
    n = len(out)
    w = path_spec(write_step, write_rmin, write_rmax)
    offsets = np.zeros(n + 1, dtype=np.int64)
    traced = np.zeros(n, dtype=np.uint8)
    h_rows, total, st = C.c_void_p(), C.c_int64(), Stats()
    capi.check(L, L.kr_trace_paths_f64(C.byref(params), C.byref(w), _ptr(out), n, _ptr(offsets), _ptr(traced), C.byref(h_rows), C.byref(total), C.byref(st)),
               "kr_trace_paths")
    try:
        rows = np.empty((total.value, 4), dtype=np.float64)
        if total.value > 0:
            C.memmove(rows.ctypes.data, h_rows.value, rows.nbytes)
    finally:
        L.kr_host_free(h_rows)
    if cartesian:
        rows = rows_to_cartesian(rows, params.spin if spin is None else spin)
    return offsets, rows, traced, out, st.as_dict()


def _path_field(v):
    # operator<< of an ofstream with setw(20), scientific, precision 8 (src/include/text_output.h); a NaN carries its sign
    if v != v:
        return "%20s" % ("-nan" if np.signbit(v) else "nan")
    return "%20.8e" % v


def paths_text(offsets, rows, traced):
    """The reference's trajectory file of a recording: one row per line, every field setw(20) scientific precision 8, and two blank lines after
    each ray that was traced (raytracer.cpp:99) -- also after one that wrote no row."""
    parts = []
    for i in range(len(offsets) - 1):
        if not traced[i]:
            continue
        for row in rows[offsets[i]:offsets[i + 1]].tolist():
            parts.append("".join(_path_field(v) for v in row) + "\n")
        parts.append("\n\n")
    return "".join(parts)


VOLUME_PLANES = ("count", "time", "redshift")
VOLUME_TALLIES = ("rows", "in_grid", "deposits", "bad_g")


def volume_map_struct(r0, rmax, nr, ntheta, nphi, logbin, V=-1.0, mode=0, reverse=0, projradius=1, motion=0):
    """A kr_volume_map with the bin widths of Mapper's constructor (src/mapper/mapper.cpp:14-16), from the C library as it computes them:
    dr = exp(log(rmax / r0) / (nr - 1)) or (rmax - r0) / (nr - 1), dtheta = (pi / 2) / (ntheta - 1), dphi = 2 pi / (nphi - 1) -- n cells of that
    width, so the last cell starts at the upper bound.  An axis of ONE cell (where the constructor divides by zero) spans the whole range:
    rmax / r0 or rmax - r0, pi / 2, 2 pi.  mode 0: one deposit per passage of a cell, 1: one per row; V, reverse, projradius, motion: as redshift()."""
    m = capi.VolumeMap()
    m.r_min = float(r0)
    m.dr = math.exp(math.log(rmax / r0) / max(nr - 1, 1)) if logbin else (rmax - r0) / max(nr - 1, 1)
    m.dtheta = (math.pi / 2) / max(ntheta - 1, 1)
    m.dphi = (2 * math.pi) / max(nphi - 1, 1)
    m.V = float(V)
    m.nr, m.ntheta, m.nphi, m.logbin = int(nr), int(ntheta), int(nphi), int(bool(logbin))
    m.mode, m.reverse, m.projradius, m.motion = int(mode), int(reverse), int(projradius), int(motion)
    return m


def _volume_layout(m, words=None):
    return _layout([(k, (m.nr, m.ntheta, m.nphi)) for k in VOLUME_PLANES], [(k, _rounded) for k in VOLUME_TALLIES], words)


def volume_words(m):
    """Length of a volume map buffer: three planes of nr ntheta nphi cells and four tallies (include/kr_trace.h, kr_trace_volume_*)."""
    return _volume_layout(m)


def volume_from_words(m, words):
    """The volume map buffer as a dict: count / time / redshift (raw sums, shaped (nr, ntheta, nphi); count stays a double array of whole numbers)
    and the tallies rows / in_grid / deposits / bad_g (ints)."""
    return _volume_layout(m, words)


def cell_volume(m, spin):
    """Mapper::calculate_volume (src/mapper/mapper.cpp:311-338) on the host: sqrt(-g_rr g_thth g_phph) dr dtheta dphi at the lower corner of every
    cell, shaped (nr, ntheta, nphi).  O(cells)."""
    a = float(spin)
    ir = np.arange(m.nr, dtype=np.float64)
    r = (m.r_min * np.power(m.dr, ir) if m.logbin else m.r_min + m.dr * ir)[:, None]
    this_dr = r * (m.dr - 1) if m.logbin else np.full_like(r, m.dr)
    theta = (np.arange(m.ntheta, dtype=np.float64) * m.dtheta)[None, :]
    rhosq = r * r + (a * np.cos(theta)) * (a * np.cos(theta))
    delta = r * r - 2 * r + a * a
    sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * np.sin(theta) * np.sin(theta)
    e2psi = sigmasq * np.sin(theta) * np.sin(theta) / rhosq
    grr, gthth, gphph = -rhosq / delta, -rhosq, -e2psi
    with np.errstate(invalid="ignore"):
        vol = np.sqrt(-1 * grr * gthth * gphph) * this_dr * m.dtheta * m.dphi
    return np.repeat(vol[:, :, None], m.nphi, axis=2)


def trace_volume(params, rays, m):
    """kr_trace_volume_f64 on a host array of Ray<double> records (Euler / RK4, strict arithmetic): the rays are integrated as trace(flags = 0)
    integrates them and binned into the grid of `m` as they step.  Returns a dict: count / time / redshift shaped (nr, ntheta, nphi), the tallies
    rows / in_grid / deposits / bad_g, "rays" (the final records, as trace() gives them) and "stats"."""
    _rays_arg(rays, capi.RAY_F64)
    out = rays.copy()
    words = np.zeros(volume_words(m))
    st = Stats()
    capi.check(lib(), lib().kr_trace_volume_f64(C.byref(params), C.byref(m), _ptr(out), len(out), _ptr(words), C.byref(st)), "kr_trace_volume")
    res = volume_from_words(m, words)
    res.update(rays=out, stats=st.as_dict())
    return res


def volume_map(sources, params, m, reverse=0, projradius=0):
    """The map of an extended source as a sum over point sources, resident on the device: for every PointSourceSpec the rays with their emitted
    energy (kr_pointsource_init_emit_dev_f64: redshift_start with the source's own V) -> kr_trace_volume_dev_f64, all adding into ONE map.
    Returns the sums count / time / redshift, the tallies, "mean_time" = time / count and "mean_redshift" = redshift / count (Mapper::average_rays;
    NaN in cells no ray crossed), "num_rays" (rays traced) and "stats" (summed over the sources)."""
    L = lib()
    nw = volume_words(m)
    stats = {}
    with DeviceScope(L) as dev:
        d_map = dev.zeros(nw * 8)
        for s in sources:
            n = pointsource_count(s)[0]
            if n <= 0:
                raise KrError("volume_map: empty ray grid")
            with DeviceScope(L) as one:                          # a source's rays are freed before the next source's are allocated
                d_rays = one.alloc(n * capi.RAY_F64.itemsize)
                capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(s), 0, 1, s.V, int(reverse), int(projradius), d_rays, n, None), "kr_pointsource_init_emit")
                st = Stats()
                capi.check(L, L.kr_trace_volume_dev_f64(C.byref(params), C.byref(m), d_rays, n, d_map, None, C.byref(st)), "kr_trace_volume")
                _add_stats(stats, st.as_dict())
        res = volume_from_words(m, dev.fetch(d_map, nw))
    with np.errstate(invalid="ignore", divide="ignore"):
        res.update(mean_time=res["time"] / res["count"], mean_redshift=res["redshift"] / res["count"])
    res.update(num_rays=int(stats.get("rays_traced", 0)), stats=stats)
    return res


OBSERVE_TALLIES = ("rows", "in_grid", "lit", "contributions", "bad_g", "degenerate")


def observe_bins_struct(en0, enmax, nen, logbin_en=False, t0=0.0, tmax=0.0, nt=0):
    """A kr_observe_bins of nen energy bins over [en0, enmax) -- den = (enmax - en0) / nen, or the ratio exp(log(enmax / en0) / nen) with
    logbin_en -- and nt time bins over [t0, tmax) (nt = 0: no response)."""
    b = capi.ObserveBins()
    b.en0, b.t0 = float(en0), float(t0)
    b.den = math.exp(math.log(enmax / en0) / nen) if logbin_en else (enmax - en0) / nen
    b.dt = (tmax - t0) / nt if nt > 0 else 0.0
    b.nen, b.nt, b.logbin_en, b.pad = int(nen), int(nt), int(bool(logbin_en)), 0
    return b


def _observe_layout(b, words=None):
    return _layout([("spectrum", (b.nen,)), ("hits", (b.nen,)), ("response", (b.nen, b.nt))], [(k, _rounded) for k in OBSERVE_TALLIES], words)


def observe_words(b):
    """Length of an observe output buffer: spectrum and hits of nen bins, the nen x nt response and six tallies (include/kr_trace.h, kr_trace_observe_*)."""
    return _observe_layout(b)


def observe_from_words(b, words):
    """The observe output buffer as a dict: "energy" (the nen + 1 bin edges), spectrum, hits (a double array of whole numbers), response shaped
    (nen, nt) and the tallies rows / in_grid / lit / contributions / bad_g / degenerate (ints)."""
    i = np.arange(b.nen + 1, dtype=np.float64)
    return {"energy": b.en0 * np.power(b.den, i) if b.logbin_en else b.en0 + b.den * i, **_observe_layout(b, words)}


def _cells_arg(a, m, name):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    if a.size != m.nr * m.ntheta * m.nphi:
        raise KrError(f"trace_observe: {name} has {a.size} values, the grid has {m.nr * m.ntheta * m.nphi} cells")
    return a


def trace_observe(params, rays, m, bins, emis, kappa=None, delay=None, want_image=True):
    """kr_trace_observe_f64 on a host array of Ray<double> records (Euler / RK4, strict arithmetic): the rays are integrated as trace(flags = 0)
    integrates them and gather the emissivity `emis` (absorption `kappa`, flash delay `delay`; arrays of one value per cell of `m`) of the cells they
    cross as they step.  Returns a dict: energy / spectrum / hits / response, the six tallies, "image" (the per-ray totals, or None), "rays" (the final
    records, as trace() gives them) and "stats"."""
    _rays_arg(rays, capi.RAY_F64)
    out = rays.copy()
    emis, kappa, delay = _cells_arg(emis, m, "emis"), _cells_arg(kappa, m, "kappa"), _cells_arg(delay, m, "delay")
    if emis is None:
        raise KrError("trace_observe: emis is required")
    words = np.zeros(observe_words(bins))
    image = np.zeros(len(out)) if want_image else None
    st = Stats()
    opt = lambda a: _ptr(a) if a is not None else None      # noqa: E731
    capi.check(lib(), lib().kr_trace_observe_f64(C.byref(params), C.byref(m), C.byref(bins), _ptr(emis), opt(kappa), opt(delay), _ptr(out), len(out), _ptr(words),
                                                 opt(image), C.byref(st)), "kr_trace_observe")
    res = observe_from_words(bins, words)
    res.update(image=image, rays=out, stats=st.as_dict())
    return res


def volume_emissivity(vmap, m, spin, gamma=2.0):
    """(emis, delay) of a volume map (the dict volume_map returns), shaped (nr, ntheta, nphi): emis = count / (num_rays cell_volume) mean_redshift^-gamma,
    the expression commented out at source_tracer.cpp:257 (gamma = 2 there), and delay = mean_time (:258).  Both are 0 where nothing crossed; emis is
    also 0 in a cell of no volume (the lower corner of the first polar cell lies on the axis).  O(cells), on the host."""
    count = np.asarray(vmap["count"], dtype=np.float64)
    vol = cell_volume(m, spin)
    ok = (count > 0) & (vol > 0) & np.isfinite(vol)
    emis, delay = np.zeros(count.shape), np.zeros(count.shape)
    mean_g = vmap["redshift"][ok] / count[ok]
    emis[ok] = count[ok] / (float(vmap["num_rays"]) * vol[ok]) * np.power(mean_g, -1 * gamma)
    hit = count > 0
    delay[hit] = vmap["time"][hit] / count[hit]
    return emis, delay


def volume_spectrum(sources, plane_spec, p_source, p_plane, m, bins, gamma=2.0, kappa=None, reverse=1):
    """Corona geometry -> observed spectrum and response of the illuminated volume, resident on the device: volume_map(sources, p_source, m) ->
    volume_emissivity (host, O(cells)) -> the ImagePlane `plane_spec` built on the device with redshift_start(0, reverse)
    (kr_imageplane_init_emit_dev_f64) -> kr_trace_observe_dev_f64 with `p_plane` (the stored, negated spin of an ImagePlane) and `m` with
    reverse = `reverse` (the camera's rays run backwards).  The rays never leave the device.  kappa: one value per cell, or None.
    Returns observe_from_words(...) plus "image" shaped (nx, ny), "map" (the volume map), "emis", "delay" and "stats" (the observing trace's)."""
    L = lib()
    vmap = volume_map(sources, p_source, m)
    emis, delay = volume_emissivity(vmap, m, p_source.spin, gamma)
    n, nx, ny = imageplane_count(plane_spec)
    if n <= 0:
        raise KrError("volume_spectrum: empty ray grid")
    mo = capi.VolumeMap.from_buffer_copy(m)
    mo.reverse = int(reverse)
    cells = [_cells_arg(emis, m, "emis"), _cells_arg(kappa, m, "kappa"), _cells_arg(delay, m, "delay")]
    nw = observe_words(bins)
    st = Stats()
    with DeviceScope(L) as dev:
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        d_out = dev.alloc(nw * 8)
        d_image = dev.alloc(n * 8)
        dev.zero(d_out, nw * 8)
        d_emis, d_kappa, d_delay = (dev.upload(a) if a is not None else None for a in cells)
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(plane_spec), 0, 1, 0.0, int(reverse), 0, d_rays, n, None), "kr_imageplane_init_emit")
        capi.check(L, L.kr_trace_observe_dev_f64(C.byref(p_plane), C.byref(mo), C.byref(bins), d_emis, d_kappa, d_delay, d_rays, n, d_out, d_image, None, C.byref(st)),
                   "kr_trace_observe")
        res = observe_from_words(bins, dev.fetch(d_out, nw))
        image = dev.fetch(d_image, n)
    res.update(image=image.reshape(nx, ny), map=vmap, emis=emis, delay=delay, stats=st.as_dict())
    return res


def crossing_spec(max_crossings=4, stop_when_full=True, V=-1.0, reverse=0, projradius=0, motion=0):
    """A kr_crossing_spec: up to max_crossings (1..16) equatorial crossings stored per ray; stop_when_full: a ray ends with the iteration that made its
    last storable crossing; V, reverse, projradius, motion: the emitter on the plane, as redshift() takes them (V = -1: Keplerian at the crossing)."""
    s = capi.CrossingSpec()
    s.V, s.max_crossings, s.stop_when_full = float(V), int(max_crossings), int(bool(stop_when_full))
    s.reverse, s.projradius, s.motion, s.pad = int(reverse), int(projradius), int(motion), 0
    return s


def trace_crossings(params, rays, spec):
    """kr_trace_crossings_f64 on a host array of Ray<double> records (Euler / RK4, strict arithmetic): the rays are integrated as trace(flags = 0)
    integrates them and every meeting with the equatorial plane is recorded (include/kr_trace.h has the rule).  Returns a dict: "rows" shaped
    (n, M, 4), {r_c, phi_c, t_c, g} per stored crossing and NaN where a ray stored none; "seen" (n,), the crossings each ray made in this call; "rays"
    (the final records) and "stats"."""
    _rays_arg(rays, capi.RAY_F64)
    out = rays.copy()
    rows = np.full((len(out), int(spec.max_crossings), 4), np.nan)
    seen = np.zeros(len(out), dtype=np.int32)
    st = Stats()
    capi.check(lib(), lib().kr_trace_crossings_f64(C.byref(params), C.byref(spec), _ptr(out), len(out), _ptr(rows), _ptr(seen), C.byref(st)), "kr_trace_crossings")
    return {"rows": rows, "seen": seen, "rays": out, "stats": st.as_dict()}


def _crossing_planes(dev, bins, max_crossings, order, lo, hi, d_rays, d_rows, d_seen, n, d_planes):
    """One order's image planes from device-resident crossings, through the scratch d_planes (zeroed here): the dict of image_planes_from_words."""
    L, nw = dev.lib, image_words(bins)
    dev.zero(d_planes, nw * 8)
    capi.check(L, L.kr_reduce_crossing_image_dev_f64(C.byref(bins), int(max_crossings), int(order), lo, hi, d_rays, d_rows, d_seen, n, d_planes, None),
               "kr_reduce_crossing_image")
    return image_planes_from_words(dev.fetch(d_planes, nw), bins.img_nx, bins.img_ny)


def reduce_crossing_image(bins, rays, rows, seen, order, lo=-np.pi, hi=np.pi):
    """The image of one order from what trace_crossings returned (kr_reduce_crossing_image_dev_f64): order >= 0 takes every ray's crossing `order`,
    order = -1 (the opaque disc) its first stored crossing inside [r_isco, r_disc).  Returns the dict of image_planes_from_words (raw sums, as
    reduce_image gives them)."""
    _rays_arg(rays, capi.RAY_F64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    seen = np.ascontiguousarray(seen, dtype=np.int32)
    n = len(rays)
    if rows.ndim != 3 or rows.shape[0] != n or rows.shape[2] != 4 or seen.shape != (n,):
        raise KrError("reduce_crossing_image: rows must be shaped (n, M, 4) and seen (n,)")
    with DeviceScope(lib()) as dev:
        d_rays, d_rows, d_seen = dev.upload(rays), dev.upload(rows), dev.upload(seen)
        return _crossing_planes(dev, bins, rows.shape[1], order, lo, hi, d_rays, d_rows, d_seen, n, dev.alloc(image_words(bins) * 8))


def order_images(imageplane_spec, params, bins, spec, orders, lo=-np.pi, hi=np.pi):
    """The order-resolved images of an equatorial disc, resident on the device: ImagePlane ctor + redshift_start(0, spec.reverse)
    (kr_imageplane_init_emit_dev_f64) -> kr_trace_crossings_dev_f64 with `params` (the stored, negated spin of an ImagePlane; theta_max = 0 lets the
    rays run on through the plane) -> kr_reduce_crossing_image_dev_f64 once per entry of `orders` (-1: the opaque disc).  The rays never leave the
    device.  Returns {"images": {order: the dict of image_planes_from_words}, "seen_histogram": how many rays made 0, 1, .. crossings,
    "stats": the trace's}."""
    L = lib()
    n, _, _ = imageplane_count(imageplane_spec)
    if n <= 0:
        raise KrError("order_images: empty ray grid")
    M = int(spec.max_crossings)
    st = Stats()
    images = {}
    with DeviceScope(L) as dev:
        d_rays, d_rows, d_seen = dev.alloc(n * capi.RAY_F64.itemsize), dev.alloc(n * M * 32), dev.alloc(n * 4)
        d_planes = dev.alloc(image_words(bins) * 8)
        capi.check(L, L.kr_imageplane_init_emit_dev_f64(C.byref(imageplane_spec), 0, 1, 0.0, int(spec.reverse), 0, d_rays, n, None), "kr_imageplane_init_emit")
        capi.check(L, L.kr_trace_crossings_dev_f64(C.byref(params), C.byref(spec), d_rays, n, d_rows, d_seen, None, C.byref(st)), "kr_trace_crossings")
        for order in orders:
            images[int(order)] = _crossing_planes(dev, bins, M, order, lo, hi, d_rays, d_rows, d_seen, n, d_planes)
        seen = dev.fetch(d_seen, n, np.int32)
    return {"images": images, "seen_histogram": np.bincount(seen), "stats": st.as_dict()}


# ---- HEALPix point source and the fate map of its sky (include/kr_trace.h: kr_healpix_source, kr_healpix_map) ----------------------------------
HEALPIX_PLANES = ("class", "r", "theta", "phi", "g", "t", "emis")
HEALPIX_TALLIES = ("live", "disc", "escape", "lost", "self")


def healpix_spec(pos, V, spin, order, motion=0, basis=0, rays_per_pixel=5, unit_center=0, E=1.0, disc_source=0):
    """A kr_healpix_source: the reference's HealpixPointSource(pos, V, spin, order, motion, basis), five rays per pixel or the centres alone;
    disc_source = 1 is its set_disc_source(): rays that start into the disc under the source are unused slots (steps = -1)."""
    s = capi.HealpixSource()
    for i in range(4):
        s.pos[i] = pos[i]
    s.V, s.spin, s.E = V, spin, E
    s.order, s.motion, s.basis, s.rays_per_pixel, s.unit_center = int(order), int(motion), int(basis), int(rays_per_pixel), int(unit_center)
    s.disc_source = int(disc_source)
    return s


def healpix_count(spec):
    """(rays, pixels) of the source; raises for a spec the library refuses."""
    npix = C.c_int64()
    n = lib().kr_healpix_count(C.byref(spec), C.byref(npix))
    if n < 0:
        capi.check(lib(), int(n), "kr_healpix_count")
    return int(n), int(npix.value)


def healpix_vectors(order, first_pix=0, stride=1, count=None, unit_center=0):
    """kr_healpix_vectors_dev_f64: [count, 15] -- four corners then the centre of pixel first_pix + k stride (default: the whole sphere)."""
    L = lib()
    if count is None:
        count = (12 * 4 ** int(order) - first_pix + stride - 1) // stride if 0 <= order <= 13 else 0
    with DeviceScope(L) as dev:
        d = dev.alloc(count * 15 * 8) if count > 0 else C.c_void_p()
        capi.check(L, L.kr_healpix_vectors_dev_f64(int(order), int(unit_center), int(first_pix), int(stride), int(count), d, None), "kr_healpix_vectors")
        return dev.fetch(d, max(count, 0) * 15).reshape(-1, 15)


def healpix_init(spec, emit=True, reverse=0, first=0, stride=1, count=None):
    """The source's ray records, built on the device: with their emitted energy (kr_healpix_init_emit_dev_f64) or with emit = 0
    (kr_healpix_init_dev_f64).  first / stride count pixels; count records (default: every pixel from `first` on at that stride)."""
    L = lib()
    n, npix = healpix_count(spec)
    if count is None:
        count = spec.rays_per_pixel * ((npix - first + stride - 1) // stride)
    with DeviceScope(L) as dev:
        d = dev.alloc(count * capi.RAY_F64.itemsize) if count > 0 else C.c_void_p()
        if emit:
            capi.check(L, L.kr_healpix_init_emit_dev_f64(C.byref(spec), int(first), int(stride), int(reverse), d, int(count), None), "kr_healpix_init_emit")
        else:
            capi.check(L, L.kr_healpix_init_dev_f64(C.byref(spec), int(first), int(stride), d, int(count), None), "kr_healpix_init")
        return dev.fetch(d, max(count, 0), capi.RAY_F64)


def healpix_map_struct(npix, r_isco, r_disc, r_esc, theta_tol=0.0, source_r=0.0, source_phi=0.0, self_zone=0, rays_per_pixel=5, q1=3.0, rb1=4.0, q2=3.0,
                       rb2=10.0, q3=3.0):
    m = capi.HealpixMap()
    m.r_isco, m.r_disc, m.r_esc, m.theta_tol, m.source_r, m.source_phi = r_isco, r_disc, r_esc, theta_tol, source_r, source_phi
    m.q1, m.rb1, m.q2, m.rb2, m.q3 = q1, rb1, q2, rb2, q3
    m.npix, m.rays_per_pixel, m.self_zone = int(npix), int(rays_per_pixel), int(self_zone)
    return m


def _healpix_map_layout(m, words=None):
    return _layout([(k, (m.npix,)) for k in HEALPIX_PLANES], [(k, _rounded) for k in HEALPIX_TALLIES] + [(None, None)], words)


def healpix_map_words(m):
    """Length of the fate-map buffer: seven planes of npix and six tallies."""
    return _healpix_map_layout(m)


def healpix_map_from_words(m, words):
    """The fate-map buffer as a dict: the planes by name ("class" as int64), the tallies live / disc / escape / lost / self (ints) and the fractions
    of the live rays "disc_frac" / "escape_frac" / "lost_frac" / "self_frac" (the reference's Return / Escape / Lost, healpix_disc_source_photonfrac.cpp:111-113)."""
    out = _healpix_map_layout(m, words)
    out["class"] = np.rint(out["class"]).astype(np.int64)
    tail = np.asarray(words, dtype=np.float64)[-6:-1]                      # live, then the four fates
    with np.errstate(invalid="ignore", divide="ignore"):
        out.update(zip((k + "_frac" for k in HEALPIX_TALLIES[1:]), (tail[1:] / tail[0]).tolist()))
    return out


def reduce_healpix_map(m, rays):
    """kr_reduce_healpix_map_f64: the fate map of the host records of a whole sphere, read as they are (after range_phi() and redshift())."""
    _rays_arg(rays, capi.RAY_F64)
    out = np.zeros(healpix_map_words(m))
    capi.check(lib(), lib().kr_reduce_healpix_map_f64(C.byref(m), _ptr(rays), len(rays), _ptr(out)), "kr_reduce_healpix_map")
    return healpix_map_from_words(m, out)


def healpix_map(spec, params, m, reverse=0, projradius=0, V=-1.0, motion=0, lo=-np.pi, hi=np.pi, return_records=False):
    """The fate of every direction of a HEALPix source's sky, resident on the device: the rays with their emitted energy
    (kr_healpix_init_emit_dev_f64) -> kr_trace_dev_f64 with `params` -> range_phi + redshift(V, reverse, projradius, motion) + the classes
    (kr_post_healpix_map_dev_f64).  The rays never leave the device (return_records copies the final records back, for tests).  Returns the dict of
    healpix_map_from_words plus "stats"."""
    L = lib()
    n, npix = healpix_count(spec)
    if m.npix != npix or m.rays_per_pixel != spec.rays_per_pixel:
        raise KrError("healpix_map: the map's npix / rays_per_pixel are not the source's")
    nw = healpix_map_words(m)
    st = Stats()
    with DeviceScope(L) as dev:
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize)
        d_out = dev.zeros(nw * 8)
        capi.check(L, L.kr_healpix_init_emit_dev_f64(C.byref(spec), 0, 1, int(reverse), d_rays, n, None), "kr_healpix_init_emit")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        capi.check(L, L.kr_post_healpix_map_dev_f64(params.spin, V, int(reverse), int(projradius), int(motion), lo, hi, C.byref(m), d_rays, n, 0, 1, d_out, None),
                   "kr_post_healpix_map")
        res = healpix_map_from_words(m, dev.fetch(d_out, nw))
        res["stats"] = st.as_dict()
        if return_records:
            res["records"] = dev.fetch(d_rays, n, capi.RAY_F64)
    return res


def healpix_to_disc_text(res):
    """The table kr_healpix_to_disc writes for the result of healpix_map(): `pix r phi redshift emis` per pixel, every field setw(20), doubles
    scientific with precision 8 (host/include/text_output.h); a pixel whose class is not 1 (disc) is `pix nan nan nan 0`."""
    rows = []
    for pix, c in enumerate(res["class"].tolist()):
        if c == 1:
            rows.append("%20d" % pix + "".join(_path_field(float(res[k][pix])) for k in ("r", "phi", "g", "emis")) + "\n")
        else:
            rows.append("%20d%20s%20s%20s%20d\n" % (pix, "nan", "nan", "nan", 0))
    return "".join(rows)


# ---- point source with any four-velocity, and where its rays end by emission angle (include/kr_trace.h: kr_pointsource_vel_spec, kr_angdist_spec) ----
def pointsource_vel_spec(pos, u, spin, dcosalpha, dbeta, cosalpha0=-0.995, cosalphamax=0.995, beta0=-np.pi, betamax=np.pi, E=1.0, tol=100.0):
    """A kr_pointsource_vel_spec: the reference's PointSourceVel(pos, u, spin, tol, dcosalpha, dbeta, cosalpha0, cosalphamax, beta0, betamax, E); u is the
    contravariant four-velocity (u^t, u^r, u^theta, u^phi) and need not be normalised (four_velocity() builds one from coordinate velocities)."""
    s = capi.PointSourceVelSpec()
    for i in range(4):
        s.pos[i], s.u[i] = pos[i], u[i]
    s.spin, s.tol, s.E = spin, tol, E
    s.dcosalpha, s.dbeta, s.cosalpha0, s.cosalphamax, s.beta0, s.betamax = dcosalpha, dbeta, cosalpha0, cosalphamax, beta0, betamax
    return s


def four_velocity(pos, spin, omega=None, dr_dt=0.0, dtheta_dt=0.0):
    """The normalised four-velocity u^t (1, dr/dt, dtheta/dt, omega) of an emitter at pos = (t, r, theta, phi) with the given coordinate velocities;
    omega=None takes the frame-dragging rate of the zero-angular-momentum observer, -g_tphi / g_phiphi.  Raises ValueError for a velocity that is
    not timelike (g(u, u) <= 0 for u = (1, dr/dt, dtheta/dt, omega))."""
    r, theta, a = float(pos[1]), float(pos[2]), float(spin)
    st, ct = math.sin(theta), math.cos(theta)
    rhosq = r * r + (a * ct) * (a * ct)
    delta = r * r - 2 * r + a * a
    sigmasq = (r * r + a * a) * (r * r + a * a) - a * a * delta * st * st
    e2nu, e2psi, w = rhosq * delta / sigmasq, sigmasq * st * st / rhosq, 2 * a * r / sigmasq
    g00, g03, g11, g22, g33 = e2nu - w * w * e2psi, w * e2psi, -rhosq / delta, -rhosq, -e2psi
    if omega is None:
        omega = w
    norm = g00 + 2 * g03 * omega + g11 * dr_dt * dr_dt + g22 * dtheta_dt * dtheta_dt + g33 * omega * omega
    if not norm > 0:
        raise ValueError(f"four_velocity: (1, {dr_dt}, {dtheta_dt}, {omega}) is not timelike at r = {r}, theta = {theta} (g(u, u) = {norm})")
    ut = 1 / math.sqrt(norm)
    return (ut, ut * dr_dt, ut * dtheta_dt, ut * omega)


def pointsource_vel_count(spec):
    """(rays, n_cosalpha, n_beta) of the source; raises for a grid the library refuses."""
    nc, nb = C.c_int32(), C.c_int32()
    n = lib().kr_pointsource_vel_count(C.byref(spec), C.byref(nc), C.byref(nb))
    if n < 0:
        capi.check(lib(), capi.KR_EINVAL, "kr_pointsource_vel_count")
    return int(n), nc.value, nb.value


def pointsource_vel_tetrad(spec):
    """The emitter's tetrad [leg, (t, r, theta, phi)] as the library solves it on the host (no device needed)."""
    out = np.zeros((4, 4))
    capi.check(lib(), lib().kr_pointsource_vel_tetrad(C.byref(spec), _ptr(out)), "kr_pointsource_vel_tetrad")
    return out


def pointsource_vel_init(spec, emit=False):
    """The source's ray records, built on the device: with emit = 0 (kr_pointsource_vel_init_dev_f64) or with the photon energy in the emitter's own
    frame (kr_pointsource_vel_init_emit_dev_f64)."""
    L = lib()
    n = pointsource_vel_count(spec)[0]
    with DeviceScope(L) as dev:
        d = dev.alloc(n * capi.RAY_F64.itemsize) if n > 0 else C.c_void_p()
        if emit:
            capi.check(L, L.kr_pointsource_vel_init_emit_dev_f64(C.byref(spec), d, n, None), "kr_pointsource_vel_init_emit")
        else:
            capi.check(L, L.kr_pointsource_vel_init_dev_f64(C.byref(spec), d, n, None), "kr_pointsource_vel_init")
        return dev.fetch(d, n, capi.RAY_F64)


ANGDIST_CLASSES = ("escape", "return", "lost")
ANGDIST_ANGLES = ("alpha", "beta", "norm", "az")
ANGDIST_TALLIES = ("ray_count", "escape", "return", "lost", "other", "skipped", "out_of_range", "bad_g")


def angdist_spec(r_isco, r_disc, r_esc, dangle=0.1, source_r=0.0, source_phi=0.0, plane_iso=1, limb=0, weight_norm=1, labels=0):
    """A kr_angdist_spec; source_r = 0 (the default) switches the self-zone of kr_return_bins off, as in the reference's program.  labels: whose
    (alpha, beta) the records carry -- 0 for a PointSource (pointsource_init), 1 for a PointSourceVel (pointsource_vel_init, source_angdist), whose
    beta is a quarter turn ahead of PointSource's."""
    sp = capi.AngdistSpec()
    c = sp.cls
    c.r_isco, c.r_disc, c.r_esc, c.source_r, c.source_phi = r_isco, r_disc, r_esc, source_r, source_phi
    c.plane_iso, c.limb, c.weight_norm, c.pad = int(plane_iso), int(limb), int(weight_norm), 0
    sp.dangle, sp.labels, sp.pad = dangle, int(labels), 0
    return sp


def angdist_nangle(spec):
    n = lib().kr_angdist_nangle(C.byref(spec))
    if n < 0:
        capi.check(lib(), capi.KR_EINVAL, "kr_angdist_nangle")
    return n


def _angdist_layout(nangle, words=None):
    planes = [(f"{c}_{a}", (nangle,)) for c in ANGDIST_CLASSES for a in ANGDIST_ANGLES] + [("total_norm", (nangle,)), ("total_az", (nangle,))]
    tallies = [(k if k not in ANGDIST_CLASSES else k + "_sum", float if q < 4 else _rounded) for q, k in enumerate(ANGDIST_TALLIES)]
    return _layout(planes, tallies, words)


def angdist_words(spec):
    """Length of the angular-distribution buffer: fourteen histograms of Nangle and eight tallies."""
    return _angdist_layout(angdist_nangle(spec))


def angdist_from_words(spec, words, normalise_az=False):
    """The buffer as a dict of named arrays: "<class>_<angle>" for class in escape / return / lost and angle in alpha / beta / norm / az,
    "total_norm", "total_az", the tallies ray_count, escape_sum, return_sum, lost_sum (weighted) and other, skipped, out_of_range, bad_g (ints), the
    fractions "escape_frac" / "return_frac" / "lost_frac" = class sum / ray_count, and "angle" = -pi + i dangle.  normalise_az divides the three az
    histograms by their per-bin sum, as disc_source_return_angdist.cpp:200-209 does (0 / 0 is NaN there too)."""
    nangle = angdist_nangle(spec)
    out = _angdist_layout(nangle, words)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in ANGDIST_CLASSES:
            out[c + "_frac"] = float(np.float64(out[c + "_sum"]) / np.float64(out["ray_count"]))        # no rays: NaN, as the program prints
        if normalise_az:
            total = out["escape_az"] + out["return_az"] + out["lost_az"]
            for c in ANGDIST_CLASSES:
                out[c + "_az"] = out[c + "_az"] / total
    out["angle"] = -1 * np.pi + np.arange(nangle) * spec.dangle
    return out


def angdist(params, rays, spec, V=-1.0, reverse=0, projradius=0, motion=0, lo=-np.pi, hi=np.pi, fused=True, normalise_az=False):
    """Where traced host records end, by emission angle.  fused: range_phi(lo, hi) + redshift(V, reverse, projradius, motion) + the reduction in one
    pass (kr_post_angdist_dev_f64; `rays` itself is not modified); otherwise the records are reduced as they are (kr_reduce_angdist_dev_f64).
    params gives the spin.  Returns the dict of angdist_from_words."""
    _rays_arg(rays, capi.RAY_F64)
    L = lib()
    nw, n = angdist_words(spec), len(rays)
    with DeviceScope(L) as dev:
        d_rays = dev.upload(rays) if n > 0 else C.c_void_p()
        d_out = dev.zeros(nw * 8)
        if fused:
            capi.check(L, L.kr_post_angdist_dev_f64(params.spin, V, int(reverse), int(projradius), int(motion), lo, hi, C.byref(spec), d_rays, n, d_out, None),
                       "kr_post_angdist")
        else:
            capi.check(L, L.kr_reduce_angdist_dev_f64(C.byref(spec), d_rays, n, d_out, None), "kr_reduce_angdist")
        return angdist_from_words(spec, dev.fetch(d_out, nw), normalise_az)


def source_angdist(vel_spec, params, angdist_spec, V=-1.0, reverse=0, projradius=0, motion=0, lo=-np.pi, hi=np.pi, normalise_az=False, return_records=False):
    """From an emitter's geometry to the histograms of where its light ends, inside one DeviceScope: kr_pointsource_vel_init_emit_dev_f64 ->
    kr_trace_dev_f64 with `params` -> kr_post_angdist_dev_f64.  The records never leave the device (return_records copies the final ones back, for
    tests).  vel_spec may also be a PointSourceSpec -- the orbiting emitter of the reference's program, built with its own emitted energy
    (kr_pointsource_init_emit_dev_f64); the angdist_spec's labels must say which of the two the records come from.  Returns the dict of
    angdist_from_words plus "stats"."""
    L = lib()
    orbital = isinstance(vel_spec, capi.PointSourceSpec)
    if angdist_spec.labels != (0 if orbital else 1):
        raise KrError("source_angdist: angdist_spec.labels must be 0 for a PointSourceSpec and 1 for a PointSourceVelSpec")
    n = pointsource_count(vel_spec)[0] if orbital else pointsource_vel_count(vel_spec)[0]
    nw = angdist_words(angdist_spec)
    st = Stats()
    with DeviceScope(L) as dev:
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize) if n > 0 else C.c_void_p()
        d_out = dev.zeros(nw * 8)
        if orbital:
            capi.check(L, L.kr_pointsource_init_emit_dev_f64(C.byref(vel_spec), 0, 1, vel_spec.V, int(reverse), int(projradius), d_rays, n, None), "kr_pointsource_init_emit")
        else:
            capi.check(L, L.kr_pointsource_vel_init_emit_dev_f64(C.byref(vel_spec), d_rays, n, None), "kr_pointsource_vel_init_emit")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        capi.check(L, L.kr_post_angdist_dev_f64(params.spin, V, int(reverse), int(projradius), int(motion), lo, hi, C.byref(angdist_spec), d_rays, n, d_out, None),
                   "kr_post_angdist")
        res = angdist_from_words(angdist_spec, dev.fetch(d_out, nw), normalise_az)
        res["stats"] = st.as_dict()
        if return_records:
            res["records"] = dev.fetch(d_rays, n, capi.RAY_F64)
    return res


def angdist_text(res):
    """The table kr_angdist writes for a result of angdist() / source_angdist() made with normalise_az=True: `angle` and the alpha, beta, norm, az
    columns of escape, return, lost per bin, every field setw(20) scientific with precision 8 (host/include/text_output.h)."""
    cols = [res["angle"]] + [res[f"{c}_{a}"] for c in ANGDIST_CLASSES for a in ANGDIST_ANGLES]
    return "".join("".join(_path_field(float(col[i])) for col in cols) + "\n" for i in range(len(res["angle"])))


# ---- the source-to-observer link: the direct continuum by observer inclination (include/kr_trace.h, kr_observer_spec) ----
OBSERVER_PLANES = ("count", "sum_w", "sum_ws", "sum_wt")
OBSERVER_TALLIES = ("ray_count", "return", "escape", "lost", "other", "binned", "outside_mu", "outside_time", "inbound", "bad_g")


def observer_spec(spin, r_isco, r_disc, r_esc, nmu=20, mu0=0.0, dmu=None, gamma=0.0, dist=0.0, t0=0.0, dt=0.0, nt=0, source_r=0.0, source_phi=0.0):
    """A kr_observer_spec.  spin: the spin the records were traced with.  nmu bins of cos(theta_obs) from mu0 in steps of dmu (default: (1 - mu0) / nmu,
    the bins end at the pole).  gamma: the photon index of the weight shift^gamma (0: solid-angle counts).  dist: the radius of the reference sphere
    of the arrival time, the image plane's dist (0: the records' t as it is).  nt rows of dt from t0 (nt = 0: no time axis).  source_r = 0 (the
    default) switches the self-zone of kr_return_bins off."""
    sp = capi.ObserverSpec()
    c = sp.cls
    c.r_isco, c.r_disc, c.r_esc, c.source_r, c.source_phi = r_isco, r_disc, r_esc, source_r, source_phi
    c.plane_iso, c.limb, c.weight_norm, c.pad = 0, 0, 0, 0
    sp.spin, sp.mu0, sp.dmu = spin, mu0, dmu if dmu is not None else (1.0 - mu0) / nmu
    sp.t0, sp.dt, sp.dist, sp.gamma, sp.nmu, sp.nt = t0, dt, dist, gamma, int(nmu), int(nt)
    return sp


def _observer_layout(spec, words=None):
    return _layout([(k, (spec.nmu,)) for k in OBSERVER_PLANES] + [("hist", (spec.nmu, spec.nt))], [(k, _rounded) for k in OBSERVER_TALLIES], words)


def observer_words(spec):
    """Length of the buffer of kr_post_observer_dev_f64 / kr_reduce_observer_dev_f64: four planes of nmu, nmu rows of nt, ten tallies."""
    return _observer_layout(spec)


def observer_from_words(spec, words):
    """The buffer as a dict: count (int64), sum_w, sum_ws, sum_wt (nmu each), hist (nmu, nt), the ten tallies (ints), `mu` (the centres of the
    inclination bins), `time` (the centres (j + 0.5) dt of the rows, counted from t0) and the bin description mu0, dmu, t0, dt that the helpers
    observer_flux / direct_arrival read."""
    out = _observer_layout(spec, words)
    out["count"] = np.rint(out["count"]).astype(np.int64)
    out["mu"] = spec.mu0 + (np.arange(spec.nmu) + 0.5) * spec.dmu
    out["time"] = (np.arange(spec.nt) + 0.5) * spec.dt
    out.update(mu0=spec.mu0, dmu=spec.dmu, t0=spec.t0, dt=spec.dt)
    return out


def reduce_observer(spec, rays):
    """kr_reduce_observer_f64: the link of host ray records read as they are (after range_phi(), for a source with a self-zone)."""
    _rays_arg(rays, capi.RAY_F64)
    out = np.zeros(observer_words(spec))
    capi.check(lib(), lib().kr_reduce_observer_f64(C.byref(spec), _ptr(rays), len(rays), _ptr(out)), "kr_reduce_observer")
    return observer_from_words(spec, out)


def _source_init(what, L, source_spec, reverse, projradius):
    """(n, init) of a source: its ray count and init(d_rays), the call that builds its rays with their emitted energy on the device."""
    if isinstance(source_spec, capi.PointSourceSpec):
        n = pointsource_count(source_spec)[0]
        init = lambda d: L.kr_pointsource_init_emit_dev_f64(C.byref(source_spec), 0, 1, source_spec.V, int(reverse), int(projradius), d, n, None)      # noqa: E731
    elif isinstance(source_spec, capi.PointSourceVelSpec):
        n = pointsource_vel_count(source_spec)[0]
        init = lambda d: L.kr_pointsource_vel_init_emit_dev_f64(C.byref(source_spec), d, n, None)      # noqa: E731
    elif isinstance(source_spec, capi.HealpixSource):
        n = healpix_count(source_spec)[0]
        init = lambda d: L.kr_healpix_init_emit_dev_f64(C.byref(source_spec), 0, 1, int(reverse), d, n, None)      # noqa: E731
    else:
        raise KrError(f"{what}: source_spec must be a PointSourceSpec, a PointSourceVelSpec or a HealpixSource")
    return n, init


def source_to_observer(source_spec, params, spec, V=-1.0, reverse=0, projradius=0, motion=0, lo=-np.pi, hi=np.pi, return_records=False):
    """From a source's geometry to its direct continuum by observer inclination, resident on the device: the rays with their emitted energy
    (kr_pointsource_init_emit_dev_f64 for a PointSourceSpec, kr_pointsource_vel_init_emit_dev_f64 for a PointSourceVelSpec,
    kr_healpix_init_emit_dev_f64 for a HealpixSource) -> kr_trace_dev_f64 with `params` (KR_STOP_THETA to the disc plane, r_max beyond the spec's
    r_esc) -> range_phi + redshift(V, reverse, projradius, motion) + the link (kr_post_observer_dev_f64).  The records never leave the device
    (return_records copies the final ones back, for tests).  Returns the dict of observer_from_words plus "stats"."""
    L = lib()
    if spec.spin != params.spin:
        raise KrError("source_to_observer: spec.spin is not the spin of params")
    n, init = _source_init("source_to_observer", L, source_spec, reverse, projradius)
    sized = 1 <= spec.nmu <= 4096 and 0 <= spec.nt and spec.nmu * (4 + spec.nt) <= 1 << 24        # (the pass refuses the rest: it gets a null buffer)
    nw = observer_words(spec) if sized else 0
    st = Stats()
    with DeviceScope(L) as dev:
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize) if n > 0 else C.c_void_p()
        d_out = dev.zeros(nw * 8) if nw else C.c_void_p()
        capi.check(L, init(d_rays), "source_to_observer: source + emitted energy")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        capi.check(L, L.kr_post_observer_dev_f64(params.spin, V, int(reverse), int(projradius), int(motion), lo, hi, C.byref(spec), d_rays, n, d_out, None),
                   "kr_post_observer")
        res = observer_from_words(spec, dev.fetch(d_out, nw))
        res["stats"] = st.as_dict()
        if return_records:
            res["records"] = dev.fetch(d_rays, n, capi.RAY_F64)
    return res


def observer_flux(res):
    """Per inclination bin, the direct flux relative to an isotropic source in flat space: (sum_w / ray_count) / (dmu / 2) -- the share of the source's
    rays that reaches the bin over the share of the sphere the bin covers.  1 in flat space at gamma = 0.  (0 / 0 without rays: NaN.)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.asarray(res["sum_w"], dtype=np.float64) / np.float64(res["ray_count"])) / (res["dmu"] / 2)


def reflection_fraction(res):
    """R_f of the system: the rays that return to the disc over those that escape (unweighted counts; no escaping ray: inf or NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(res["return"]) / np.float64(res["escape"]))


def direct_arrival(res, inc_deg):
    """The direct continuum as an observer at inclination inc_deg sees it, from the bin that holds cos(inc): {"bin", "t0": sum w t_ref / sum w -- the
    instant capi.response_model(..., t0=...) and kr_reverb_response's t0 key take --, "shift": sum w shift / sum w, "flux": observer_flux there, "hist":
    the bin's time row}.  Raises KrError for an inclination outside the bins (the index rule of the pass: -1 < (cos(inc) - mu0) / dmu < nmu) and for
    a bin without rays."""
    nmu = len(res["sum_w"])
    q = (math.cos(math.radians(inc_deg)) - res["mu0"]) / res["dmu"]
    if not (q > -1 and q < nmu):
        raise KrError(f"direct_arrival: cos({inc_deg} deg) is outside the {nmu} inclination bins from mu0 = {res['mu0']} in steps of {res['dmu']}")
    i = int(q)
    sw = float(res["sum_w"][i])
    if not sw > 0:
        raise KrError(f"direct_arrival: no direct ray in inclination bin {i}")
    return {"bin": i, "t0": float(res["sum_wt"][i]) / sw, "shift": float(res["sum_ws"][i]) / sw, "flux": float(observer_flux(res)[i]),
            "hist": np.array(res["hist"][i], dtype=np.float64)}


def observer_text(res):
    """The table kr_source_observer writes for a result of source_to_observer(): the row `# R_f` with return / escape, then per inclination bin
    `mu count flux shift t_ref` -- the bin's centre, its ray count, observer_flux, the mean shift and the mean arrival time (nan in an empty bin) --
    and the nt words of the bin's time row; every field setw(20), doubles scientific with precision 8 (host/include/text_output.h)."""
    rows = ["%20s" % "# R_f" + _path_field(reflection_fraction(res)) + "\n"]
    flux = observer_flux(res)
    for i in range(len(flux)):
        sw, any_ray = float(res["sum_w"][i]), res["count"][i] > 0
        means = [float(res[k][i]) / sw if any_ray else float("nan") for k in ("sum_ws", "sum_wt")]
        rows.append(_path_field(float(res["mu"][i])) + "%20d" % int(res["count"][i]) + "".join(_path_field(float(x)) for x in [flux[i]] + means + list(res["hist"][i]))
                    + "\n")
    return "".join(rows)


# ---- the (r, phi) illumination map of the disc (include/kr_trace.h, kr_illum_bins) ----
ILLUM_PLANES = ("count", "flux", "emis", "sum_redshift", "sum_time")
ILLUM_TALLIES = ("disc_count", "binned")
ILLUM_MAX_CELLS = 1 << 20


def _illum_layout(bins, words=None):
    return _layout([(k, (bins.rad.nr, bins.nphi)) for k in ILLUM_PLANES], [(k, _rounded) for k in ILLUM_TALLIES], words)


def _illum_sized(bins):
    return bins.rad.nr >= 1 and bins.nphi >= 1 and bins.rad.nr * bins.nphi <= ILLUM_MAX_CELLS


def illum_words(bins):
    """Length of the buffer of kr_post_illum_dev_f64 / kr_reduce_illum_dev_f64: five planes of nr x nphi and two tallies."""
    return _illum_layout(bins)


def illum_from_words(bins, words):
    """That buffer as a dict: count (int64), flux, emis, sum_redshift, sum_time (raw sums), each shaped (nr, nphi); disc_count, binned; `phi` (the
    centres of the azimuthal cells, counted from -pi) and the bin description r_min, dr, logbin, phi_shift that illumination_table reads."""
    out = _illum_layout(bins, words)
    out["count"] = np.rint(out["count"]).astype(np.int64)
    out["phi"] = -np.pi + (np.arange(bins.nphi) + 0.5) * (2 * np.pi / bins.nphi)
    out.update(r_min=bins.rad.r_min, dr=bins.rad.dr, logbin=int(bins.rad.logbin), phi_shift=bins.phi_shift)
    return out


def reduce_illum(bins, rays):
    """kr_reduce_illum_f64: the (r, phi) map of host ray records read as they are (after range_phi() and redshift())."""
    _rays_arg(rays, capi.RAY_F64)
    out = np.zeros(illum_words(bins) if _illum_sized(bins) else 1)      # (the call refuses the rest before it writes)
    capi.check(lib(), lib().kr_reduce_illum_f64(C.byref(bins), _ptr(rays), len(rays), _ptr(out)), "kr_reduce_illum")
    return illum_from_words(bins, out)


def illumination_map(source_spec, params, bins, V=-1.0, reverse=0, projradius=0, motion=0, lo=-np.pi, hi=np.pi, return_records=False):
    """From a source's geometry to the (r, phi) map of how it lights the disc, resident on the device: the rays with their emitted energy
    (kr_pointsource_init_emit_dev_f64 for a PointSourceSpec, kr_pointsource_vel_init_emit_dev_f64 for a PointSourceVelSpec,
    kr_healpix_init_emit_dev_f64 for a HealpixSource) -> kr_trace_dev_f64 with `params` (KR_STOP_THETA to the disc plane) -> range_phi +
    redshift(V, reverse, projradius, motion) + the map (kr_post_illum_dev_f64).  The records never leave the device (return_records copies the final
    ones back, for tests).
    bins.phi_shift is the orbital phase: the metric is axisymmetric, so ONE trace of the source at phi_s = 0 serves every phase delta -- the map of the
    source at phi_s = delta is this map made with phi_shift = +delta, and a table made from the phi_s = 0 map is applied to disc records with
    phi_shift = -delta.  Returns the dict of illum_from_words plus "stats"."""
    L = lib()
    n, init = _source_init("illumination_map", L, source_spec, reverse, projradius)
    nw = illum_words(bins) if _illum_sized(bins) else 0                 # (the pass refuses the rest: it gets a null buffer)
    st = Stats()
    with DeviceScope(L) as dev:
        d_rays = dev.alloc(n * capi.RAY_F64.itemsize) if n > 0 else C.c_void_p()
        d_out = dev.zeros(nw * 8) if nw else C.c_void_p()
        capi.check(L, init(d_rays), "illumination_map: source + emitted energy")
        capi.check(L, L.kr_trace_dev_f64(C.byref(params), d_rays, n, None, C.byref(st)), "kr_trace_dev")
        capi.check(L, L.kr_post_illum_dev_f64(params.spin, V, int(reverse), int(projradius), int(motion), lo, hi, C.byref(bins), d_rays, n, d_out, None),
                   "kr_post_illum")
        res = illum_from_words(bins, dev.fetch(d_out, nw))
        res["stats"] = st.as_dict()
        if return_records:
            res["records"] = dev.fetch(d_rays, n, capi.RAY_F64)
    return res


def illumination_table(res, areas):
    """The (r, phi) tables of a map (illum_from_words, illumination_map): per cell the emissivity emis = emis_sum / (areas[ir] / nphi) -- areas: the
    proper area of every annulus, nr values, e.g. surface_area(edges, r_in, 0, 0, spin, dphi=2 pi) of the flat disc or integrate_disc_area of
    host/include/disc.h -- and the mean source -> disc delay time = sum_time / count, NaN where no ray landed (a pass that reads the table leaves
    the records of such a cell out, as with a non-finite entry of a radial table).  Returns {"emis", "time"} shaped (nr, nphi) and the map's r_min, dr,
    logbin, phi_shift, nr, nphi.  Host numpy."""
    emis_sum, count = np.asarray(res["emis"], dtype=np.float64), np.asarray(res["count"])
    nr, nphi = emis_sum.shape
    areas = np.asarray(areas, dtype=np.float64)
    if areas.shape != (nr,):
        raise KrError(f"illumination_table: areas must hold one area per annulus, {nr} values")
    with np.errstate(invalid="ignore", divide="ignore"):
        emis = emis_sum / (areas / nphi)[:, None]
        time = np.where(count > 0, np.asarray(res["sum_time"], dtype=np.float64) / count, np.nan)
    return {"emis": emis, "time": time, "r_min": res["r_min"], "dr": res["dr"], "logbin": res["logbin"], "phi_shift": res["phi_shift"], "nr": nr, "nphi": nphi}


# ---- continuum spectrum of the disc (include/kr_trace.h, kr_spectrum_model) ----
def _spectrum_layout(model, words=None):
    return _layout([("flux", (model.ne,))], [("on_disc", _rounded), ("used", _rounded), ("bad_angle", _rounded), (None, None)], words)


def spectrum_words(model):
    """Length of the buffer of kr_post_spectrum_dev_f64 / kr_reduce_spectrum_dev_f64: [flux (ne) | on_disc | used | bad_angle | 0]."""
    return _spectrum_layout(model)


def spectrum_energies(model):
    """The ne energies at which the spectrum is sampled: the centres of the bins (e_min, de, log_e) -- geometric centres with log_e."""
    i = np.arange(model.ne) + 0.5
    return model.e_min * np.float64(model.de) ** i if model.log_e else model.e_min + i * model.de


def spectrum_from_words(model, words):
    """The buffer of the spectrum entry points as a dict: flux (ne), on_disc, used, bad_angle, and `energy`, the ne sampling energies."""
    out = _spectrum_layout(model, words)
    out["energy"] = spectrum_energies(model)
    return out


def reduce_spectrum(model, rays):
    """kr_reduce_spectrum_f64: the isotropic continuum spectrum of host ray records that carry their redshift."""
    _rays_arg(rays, capi.RAY_F64)
    out = np.zeros(spectrum_words(model))
    capi.check(lib(), lib().kr_reduce_spectrum_f64(C.byref(model), _ptr(rays), len(rays), _ptr(out)), "kr_reduce_spectrum")
    return spectrum_from_words(model, out)


def _spectrum_stokes_layout(model, words=None):
    return _layout([(k, (model.ne,)) for k in ("flux", "q", "u")], [("on_disc", _rounded), ("used", _rounded), ("bad_pol", _rounded), (None, None)], words)


def spectrum_stokes_words(model):
    """Length of the buffer of kr_post_spectrum_stokes_dev_f64 / kr_reduce_spectrum_stokes_dev_f64: [I | Q | U (ne each) | on_disc | used | bad_pol | 0]."""
    return _spectrum_stokes_layout(model)


def spectrum_stokes_from_words(model, words):
    """The buffer of the Stokes spectrum entry points as a dict: flux, q, u (ne each: the Stokes sums I, Q, U on the plane's own x and y axes),
    pol_degree = sqrt(q^2 + u^2) / flux and pol_angle = atan2(u, q) / 2 in radians from the x axis towards the y axis (both NaN where flux == 0),
    the tallies on_disc, used, bad_pol, and `energy`, the ne sampling energies."""
    out = _spectrum_stokes_layout(model, words)
    out["energy"] = spectrum_energies(model)
    with np.errstate(all="ignore"):
        lit = out["flux"] != 0
        safe = np.where(lit, out["flux"], 1.0)
        out["pol_degree"] = np.where(lit, np.hypot(out["q"], out["u"]) / safe, np.nan)
        out["pol_angle"] = np.where(lit, 0.5 * np.arctan2(out["u"], out["q"]), np.nan)
    return out


def reduce_spectrum_stokes(model, rays, spin, inc_deg, pol, limb=None):
    """kr_reduce_spectrum_stokes_f64: the Stokes spectra I, Q, U of the continuum from host ray records of an image plane that carry their redshift.
    spin: the true spin (the a of the redshift pass with reverse = 1); inc_deg: the plane's inclination; pol, limb: as for stokes_image.  Keplerian gas
    (V = -1), projradius 0."""
    _rays_arg(rays, capi.RAY_F64)
    law, plaw = capi.limb_law(limb if limb is not None else "isotropic"), capi.pol_law(pol)
    out = np.zeros(spectrum_stokes_words(model))
    capi.check(lib(), lib().kr_reduce_spectrum_stokes_f64(spin, -1.0, 1, 0, inc_deg, C.byref(model), C.byref(law), C.byref(plaw), _ptr(rays), len(rays), _ptr(out)),
               "kr_reduce_spectrum_stokes")
    return spectrum_stokes_from_words(model, out)


def plunge_flow(spin):
    """kr_plunge_flow: (r_ms, E_ms, L_ms) of the disc flow V = capi.V_PLUNGE for the metric's spin (needs no GPU)."""
    r_ms, E_ms, L_ms = C.c_double(), C.c_double(), C.c_double()
    capi.check(lib(), lib().kr_plunge_flow(float(spin), C.byref(r_ms), C.byref(E_ms), C.byref(L_ms)), "kr_plunge_flow")
    return r_ms.value, E_ms.value, L_ms.value


def plunge_velocity(spin, r):
    """kr_plunge_velocity: the flow's four-velocity (u^t, u^r, u^theta, u^phi) on the equatorial plane at r: plunging inside r_ms, the circular orbit's
    outside (needs no GPU)."""
    u = (C.c_double * 4)()
    capi.check(lib(), lib().kr_plunge_velocity(float(spin), float(r), u), "kr_plunge_velocity")
    return np.array(u[:], dtype=np.float64)


def isco_radius(spin):
    """The prograde ISCO of Bardeen, Press & Teukolsky (1972) in double precision (kr_kerr_isco keeps the reference's float-rounded intermediates)."""
    a = float(spin)
    z1 = 1 + np.cbrt((1 - a) * (1 + a)) * (np.cbrt(1 + a) + np.cbrt(1 - a))
    z2 = np.sqrt(3 * a * a + z1 * z1)
    return float(3 + z2 - np.sqrt((3 - z1) * (3 + z1 + 2 * z2)))


def novikov_thorne_flux(r, spin, r_isco=None):
    """The flux of a Novikov-Thorne disc per unit proper area of one face, for Mdot = 1 and M = 1 (G = c = 1), prograde orbits: the closed form of
    Page & Thorne (1974), in x = sqrt(r):
      F = 3 / (8 pi) [x - x0 - 1.5 a ln(x / x0) - sum_k 3 (x_k - a)^2 / (x_k prod_{j != k} (x_k - x_j)) ln((x - x_k) / (x0 - x_k))] / (x^4 (x^3 - 3 x + 2 a))
    with x0 = sqrt(r_isco), x_1,2 = 2 cos((acos(a) -+ pi) / 3), x_3 = -2 cos(acos(a) / 3), the roots of x^3 - 3 x + 2 a.  Exactly 0 at r_isco (default:
    isco_radius(spin)), NaN inside it."""
    a = float(spin)
    r = np.asarray(r, dtype=np.float64)
    x0 = np.sqrt(isco_radius(a) if r_isco is None else float(r_isco))
    ac = np.arccos(a)
    roots = [2 * np.cos((ac - np.pi) / 3), 2 * np.cos((ac + np.pi) / 3), -2 * np.cos(ac / 3)]
    with np.errstate(all="ignore"):
        x = np.sqrt(r)
        bracket = x - x0 - 1.5 * a * np.log(x / x0)
        for k, xk in enumerate(roots):
            others = [xj for j, xj in enumerate(roots) if j != k]
            bracket = bracket - 3 * (xk - a) ** 2 / (xk * (xk - others[0]) * (xk - others[1])) * np.log((x - xk) / (x0 - xk))
        F = 3 / (8 * np.pi) * bracket / (x ** 4 * (x ** 3 - 3 * x + 2 * a))
        return np.where(x >= x0, F, np.nan)


# CODATA 2018 / IAU 2015 values, cgs
K_B_KEV_PER_K = 8.617333262e-8
SIGMA_SB_CGS = 5.670374419e-5
G_CGS = 6.67430e-8
C_CGS = 2.99792458e10
M_SUN_G = 1.98841e33


def thermal_kt_table(spin, r_min, dr, nr, mass_msun, mdot_g_s, f_col=1.0, logbin=True):
    """kT in keV of the Novikov-Thorne disc at the CENTRE of each of the nr radial bins (r_min, dr, logbin) of a kr_spectrum_model's table_kt --
    geometric centres r_min dr^(i + 0.5) with logbin, r_min + (i + 0.5) dr otherwise:  kT = k_B (F Mdot c^6 / (G^2 M^2) / sigma_SB)^(1/4), the
    EFFECTIVE temperature.  f_col does not enter the table: the model's rule applies it (I = f_col^-4 B(E, f_col kT)); the argument is accepted so
    that one set of keywords describes the disc, and is checked.  NaN inside the ISCO."""
    if not f_col > 0:
        raise KrError("thermal_kt_table: f_col must be positive")
    i = np.arange(int(nr)) + 0.5
    r = r_min * np.float64(dr) ** i if logbin else r_min + i * dr
    scale = mdot_g_s * C_CGS ** 6 / (G_CGS ** 2 * (mass_msun * M_SUN_G) ** 2)
    with np.errstate(invalid="ignore"):
        return K_B_KEV_PER_K * (novikov_thorne_flux(r, spin) * scale / SIGMA_SB_CGS) ** 0.25


def resample_spectrum(energy, counts, spec_bins):
    """A two-column rest-frame spectrum (energies ascending and positive) onto the log grid of a kr_spectrum_model: spec_bins nodes from the first to the
    last energy, each value interpolated linearly in log E between the file's neighbouring points.  Returns (s_e_min, s_de, S of shape (spec_bins,))."""
    energy, counts = np.asarray(energy, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    if len(energy) < 2 or spec_bins < 2 or not (np.diff(energy) > 0).all() or not energy[0] > 0:
        raise KrError("resample_spectrum: needs at least two ascending positive energies and spec_bins >= 2")
    s_de = float(np.exp(np.log(energy[-1] / energy[0]) / (spec_bins - 1)))
    nodes = energy[0] * s_de ** np.arange(spec_bins)
    nodes[-1] = min(nodes[-1], energy[-1])
    return float(energy[0]), s_de, np.interp(np.log(nodes), np.log(energy), counts)


def disc_spectrum(imageplane_spec, params, model, limb=None, return_records=False, V=-1.0, pol=None, surface=None):
    """The continuum spectrum of the disc seen on an image plane, resident on the device from start to finish, as the kr_disc_spectrum app runs it:
    ImagePlane ctor + redshift_start (kr_imageplane_init_emit_dev_f64) -> trace (kr_trace_dev_f64; `params` as for the image app: the stored, negated
    spin) -> redshift + range_phi + the spectrum (kr_post_spectrum_dev_f64).  model: a capi.SpectrumModel; limb: None (isotropic) or a limb law as for
    line_profile.  Only the ne + 4 words are read back (and, with return_records, the final records: for tests).  Returns spectrum_from_words(...)
    plus "stats" (the trace's kr_stats).  The flux is per image-plane pixel: multiply by dx dy / D^2 for a flux density.  V: -1 or capi.V_PLUNGE, as for
    line_profile (model.r_isco is the inner edge).
    pol: None, or a polarisation degree law as for stokes_image ((law, coeff), a name of capi.POL_LAWS or a capi.PolLaw): the Stokes spectra.  The last
    pass is then kr_post_spectrum_stokes_dev_f64 at the plane's own inclination (V = capi.V_PLUNGE is refused) and the result is
    spectrum_stokes_from_words(...) plus "stats": "q", "u", "pol_degree", "pol_angle" and "bad_pol" join it (and "bad_angle" leaves it: bad-angle is a
    subset of bad-pol).
    surface: None, or (r_in, r_out, slope, scale) / a capi.DiscSurface, as for line_profile: the continuum of the rays that landed on that surface
    (kr_post_spectrum_surface_dev_f64; trace to it with thick_disc_params(...)).  Refused together with V = capi.V_PLUNGE or pol."""
    law = capi.limb_law(limb if limb is not None else "isotropic")
    sized = 1 <= model.ne <= 4096                      # (the pass refuses the rest: it gets a null buffer)
    if surface is not None:
        sf = _surface_arg("disc_spectrum", surface, V, pol)
        words, stats, records = _imageplane_run("disc_spectrum", imageplane_spec, params, spectrum_words(model) if sized else 0, lambda L, dev, d_rays, n, d_out: capi.check(
            L, L.kr_post_spectrum_surface_dev_f64(C.byref(sf), -1 * imageplane_spec.spin, 1, -np.pi, np.pi, C.byref(model), C.byref(law), d_rays, n, d_out, None),
            "kr_post_spectrum_surface"), return_records)
        res = spectrum_from_words(model, words)
        res["stats"], res["surface"] = stats, (sf.r_in, sf.r_out, sf.slope, sf.scale)
        if return_records:
            res["records"] = records
        return res
    if pol is not None:
        plaw, spin, inc = capi.pol_law(pol), -1 * imageplane_spec.spin, imageplane_spec.inc_deg
        words, stats, records = _imageplane_run("disc_spectrum", imageplane_spec, params, spectrum_stokes_words(model) if sized else 0, lambda L, dev, d_rays, n, d_out: capi.check(
            L, L.kr_post_spectrum_stokes_dev_f64(spin, V, 1, 0, 0, -np.pi, np.pi, inc, C.byref(model), C.byref(law), C.byref(plaw), d_rays, n, d_out, None),
            "kr_post_spectrum_stokes"), return_records)
        res = spectrum_stokes_from_words(model, words)
        res["stats"] = stats
        if return_records:
            res["records"] = records
        return res
    words, stats, records = _imageplane_run("disc_spectrum", imageplane_spec, params, spectrum_words(model) if sized else 0, lambda L, dev, d_rays, n, d_out: capi.check(
        L, L.kr_post_spectrum_dev_f64(-1 * imageplane_spec.spin, V, 1, 0, 0, -np.pi, np.pi, C.byref(model), C.byref(law), d_rays, n, d_out, None), "kr_post_spectrum"),
        return_records)
    res = spectrum_from_words(model, words)
    res["stats"] = stats
    if return_records:
        res["records"] = records
    return res


def _surface_rows(res):
    """The rows "# DISCSLOP", "# DISCSCAL", "# DISCRIN" with which a program's text file opens for a disc with a surface ("" for a result without one)."""
    if "surface" not in res:
        return ""
    r_in, _, slope, scale = res["surface"]
    return "".join("%20s" % k + _path_field(float(v)) + "\n" for k, v in (("# DISCSLOP", slope), ("# DISCSCAL", scale), ("# DISCRIN", r_in)))


def line_text(res, bins, limb=None):
    """The file kr_line_profile writes for a result of line_profile(..., bins, ...): with a surface the rows of _surface_rows, with `limb` (what the
    program's limb key was given: (law, coeff) or a name) the rows "# LIMB" and "# LIMBCOEF", then one row per bin: t_mid E_mid flux count, a blank
    line after each time bin.  Every field setw(20), the numbers scientific with precision 8 (host/include/text_output.h)."""
    head = _surface_rows(res)
    if limb is not None:
        law = capi.limb_law(limb)
        head += "%20s%20d\n" % ("# LIMB", law.law) + "%20s" % "# LIMBCOEF" + _path_field(law.coeff) + "\n"
    time_axis = not (bins.nt == 1 and bins.dt <= 0)
    parts = [head]
    for j in range(bins.nt):
        t_mid = bins.t0 + (j + 0.5) * bins.dt if time_axis else float("nan")
        for i in range(bins.ne):
            lo = bins.e_min * math.pow(bins.de, i) if bins.log_e else bins.e_min + i * bins.de
            hi = bins.e_min * math.pow(bins.de, i + 1) if bins.log_e else bins.e_min + (i + 1) * bins.de
            parts.append(_path_field(t_mid) + _path_field(0.5 * (lo + hi)) + _path_field(float(res["flux"][j, i])) + "%20d\n" % int(res["count"][j, i]))
        parts.append("\n")
    return "".join(parts)


def spectrum_text(res):
    """The file kr_disc_spectrum writes for a result of disc_spectrum(): three comment rows with the tallies ("# ON_DISC", "# USED", "# BAD_ANGLE" and
    their counts), then one row per energy: E flux.  Every field setw(20), the numbers scientific with precision 8 (host/include/text_output.h).  A result
    that carries Stokes sums (disc_spectrum(pol=...)): the third tally is "# BAD_POL" and the rows are E I Q U.  A result for a disc with a surface
    (disc_spectrum(surface=...)) opens with the rows "# DISCSLOP", "# DISCSCAL", "# DISCRIN"."""
    if "q" in res:
        head = "".join("%20s%20d\n" % (f"# {k.upper()}", res[k]) for k in ("on_disc", "used", "bad_pol"))
        return head + "".join("".join(_path_field(float(v)) for v in row) + "\n" for row in zip(res["energy"], res["flux"], res["q"], res["u"]))
    head = _surface_rows(res) + "".join("%20s%20d\n" % (f"# {k.upper()}", res[k]) for k in ("on_disc", "used", "bad_angle"))
    return head + "".join(_path_field(float(e)) + _path_field(float(f)) + "\n" for e, f in zip(res["energy"], res["flux"]))


# ---- reverberation response of the disc (include/kr_trace.h, kr_response_model) ----
def _response_layout(model, words=None):
    return _layout([("resp", (model.nt, model.spec.ne))], [("on_disc", _rounded), ("used", _rounded), ("bad_angle", _rounded), ("outside", _rounded)], words)


def response_words(model):
    """Length of the buffer of kr_post_response_dev_f64 / kr_reduce_response_dev_f64: [resp (nt x ne, time-major) | on_disc | used | bad_angle | outside]."""
    return _response_layout(model)


def response_from_words(model, words):
    """The buffer of the response entry points as a dict: resp (nt, ne), the tallies on_disc, used, bad_angle, outside, `energy` (the ne sampling
    energies of model.spec) and `time`, the centres (j + 0.5) dt of the time rows, counted from t0."""
    out = _response_layout(model, words)
    m = model.spec                                          # (scalar libm arithmetic: the ENERGY axis of kr_reverb_response to the bit)
    out["energy"] = np.array([m.e_min * math.pow(m.de, i + 0.5) if m.log_e else m.e_min + (i + 0.5) * m.de for i in range(m.ne)])
    out["time"] = (np.arange(model.nt) + 0.5) * model.dt
    return out


def reduce_response(model, rays):
    """kr_reduce_response_f64: the isotropic energy-time response of host ray records that carry their redshift."""
    _rays_arg(rays, capi.RAY_F64)
    out = np.zeros(response_words(model))
    capi.check(lib(), lib().kr_reduce_response_f64(C.byref(model), _ptr(rays), len(rays), _ptr(out)), "kr_reduce_response")
    return response_from_words(model, out)


def disc_response(imageplane_spec, params, model, limb=None, return_records=False, V=-1.0, surface=None, illum=None):
    """The energy-time response of the disc seen on an image plane, resident on the device from start to finish, as the kr_reverb_response app runs it:
    ImagePlane ctor + redshift_start -> trace (`params` as for the image app: the stored, negated spin) -> redshift + range_phi + the response
    (kr_post_response_dev_f64).  model: a capi.ResponseModel; limb: None (isotropic) or a limb law as for line_profile.  Only the nt ne + 4 words are read
    back (and, with return_records, the final records: for tests).  Returns response_from_words(...) plus "stats" (the trace's kr_stats).  The response is
    per image-plane pixel: multiply by dx dy / D^2 for a flux density.  V: -1 or capi.V_PLUNGE, as for line_profile (model.spec.r_isco is the inner edge).
    surface: None, or (r_in, r_out, slope, scale) / a capi.DiscSurface, as for line_profile: the response of the rays that landed on that surface
    (kr_post_response_surface_dev_f64; trace to it with thick_disc_params(...)).  Refused together with V = capi.V_PLUNGE.
    illum: None, or an (r, phi) illumination table -- a capi.IllumTable or the dict of illumination_table -- that gives every disc cell its emissivity and
    source -> disc delay in place of powerlaw3 / the model's radial tables, which the model must then not carry (kr_post_response_illum_dev_f64).  Its
    phi_shift is the orbital phase of the source: one source trace at phi_s = 0 serves every phase (capi.illum_table).  Refused with surface or
    V = capi.V_PLUNGE.  With illum=None the calls are exactly those made without the argument."""
    law = capi.limb_law(limb if limb is not None else "isotropic")
    sized = 1 <= model.spec.ne <= 4096 and 1 <= model.nt and model.nt * model.spec.ne <= 1 << 24        # (the pass refuses the rest: it gets a null buffer)
    if illum is not None:
        table = _illum_arg("disc_response", illum, V, surface)
        words, stats, records = _imageplane_run("disc_response", imageplane_spec, params, response_words(model) if sized else 0, lambda L, dev, d_rays, n, d_out: capi.check(
            L, L.kr_post_response_illum_dev_f64(-1 * imageplane_spec.spin, V, 1, 0, 0, -np.pi, np.pi, C.byref(model), C.byref(law), C.byref(table), d_rays, n, d_out, None),
            "kr_post_response_illum"), return_records)
        res = response_from_words(model, words)
        res["stats"] = stats
        if return_records:
            res["records"] = records
        return res
    if surface is not None:
        sf = _surface_arg("disc_response", surface, V)
        words, stats, records = _imageplane_run("disc_response", imageplane_spec, params, response_words(model) if sized else 0, lambda L, dev, d_rays, n, d_out: capi.check(
            L, L.kr_post_response_surface_dev_f64(C.byref(sf), -1 * imageplane_spec.spin, 1, -np.pi, np.pi, C.byref(model), C.byref(law), d_rays, n, d_out, None),
            "kr_post_response_surface"), return_records)
        res = response_from_words(model, words)
        res["stats"], res["surface"] = stats, (sf.r_in, sf.r_out, sf.slope, sf.scale)
        if return_records:
            res["records"] = records
        return res
    words, stats, records = _imageplane_run("disc_response", imageplane_spec, params, response_words(model) if sized else 0, lambda L, dev, d_rays, n, d_out: capi.check(
        L, L.kr_post_response_dev_f64(-1 * imageplane_spec.spin, V, 1, 0, 0, -np.pi, np.pi, C.byref(model), C.byref(law), d_rays, n, d_out, None), "kr_post_response"),
        return_records)
    res = response_from_words(model, words)
    res["stats"] = stats
    if return_records:
        res["records"] = records
    return res


def gravitational_time(mass_msun):
    """G M / c^3 in seconds: the unit of the records' t, of t0 and of dt for a hole of mass_msun solar masses."""
    return G_CGS * mass_msun * M_SUN_G / C_CGS ** 3


def _band_response(resp, widths, band):
    return (np.asarray(resp, dtype=np.float64)[:, band] * np.asarray(widths, dtype=np.float64)[band]).sum(axis=1)


def _transfer(r_band, c_band, refl, dt, freqs):
    """H(f) = C + refl sinc(f dt) sum_j r[j] exp(-2 pi i f (j + 0.5) dt): the direct continuum at tau = 0 and the top-hat time rows of the response."""
    tau = (np.arange(r_band.shape[0]) + 0.5) * dt
    sinc = np.sinc(freqs * dt).reshape((-1,) + (1,) * (r_band.ndim - 1))                   # r_band: (nt,) for one band, (nt, ne) for every energy
    return c_band + refl * sinc * (np.exp(-2j * np.pi * freqs[:, None] * tau[None, :]) @ r_band)


def lag_spectra(resp, dt, widths, freqs, band, ref_band, cont=None, refl=1.0):
    """The lag-frequency spectrum of an energy band against a reference band, from an energy-time response (host numpy; O(nt ne nf)).
      r_X[j] = sum_{i in X} resp[j, i] widths[i];   C_X = sum_{i in X} cont[i] widths[i] (0 without cont): the direct continuum, arriving at tau = 0 --
      the response's t0 is the caller's choice of that instant;   H_X(f) = C_X + refl sinc(f dt) sum_j r_X[j] exp(-2 pi i f (j + 0.5) dt) with the
      normalised sinc (the top-hat row);   cross = conj(H_ref) H_X;   lag = -arg(cross) / (2 pi f), positive when the band lags the reference.
    resp: (nt, ne); widths: the ne bin widths; freqs: in 1 / (the unit of dt); band, ref_band: index arrays, slices or masks over the energies.
    Returns {"lag", "cross", "H_band", "H_ref"}, each of len(freqs)."""
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    widths = np.asarray(widths, dtype=np.float64)
    H = []
    for X in (band, ref_band):
        c = float((np.asarray(cont, dtype=np.float64)[X] * widths[X]).sum()) if cont is not None else 0.0
        H.append(_transfer(_band_response(resp, widths, X), c, refl, dt, freqs))
    cross = np.conj(H[1]) * H[0]
    with np.errstate(all="ignore"):
        lag = -np.angle(cross) / (2 * np.pi * freqs)
    return {"lag": lag, "cross": cross, "H_band": H[0], "H_ref": H[1]}


def lag_energy(resp, dt, widths, freqs, ref_band, cont=None, refl=1.0):
    """The lag-energy spectrum over a frequency range: lag_spectra with each energy as its own band; the cross-spectra are summed over `freqs` before
    the argument is taken, then divided by 2 pi mean(freqs).  Returns {"lag" (ne), "cross" (ne), "H" (nf, ne), "H_ref" (nf)}."""
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    widths = np.asarray(widths, dtype=np.float64)
    resp = np.asarray(resp, dtype=np.float64)
    c_ref = float((np.asarray(cont, dtype=np.float64)[ref_band] * widths[ref_band]).sum()) if cont is not None else 0.0
    H_ref = _transfer(_band_response(resp, widths, ref_band), c_ref, refl, dt, freqs)
    c_each = np.asarray(cont, dtype=np.float64) * widths if cont is not None else np.zeros(resp.shape[1])
    H = _transfer(resp * widths[None, :], c_each[None, :], refl, dt, freqs)                  # (nf, ne)
    cross = (np.conj(H_ref)[:, None] * H).sum(axis=0)
    lag = -np.angle(cross) / (2 * np.pi * freqs.mean())
    return {"lag": lag, "cross": cross, "H": H, "H_ref": H_ref}


# ---- orbiting hot spot on the disc (include/kr_trace.h, kr_hotspot) ----
def keplerian_omega(r, spin):
    """The angular velocity d phi / d t of a prograde circular equatorial orbit at r: 1 / (spin + r^1.5)."""
    r = np.asarray(r, dtype=np.float64)
    om = 1.0 / (spin + r * np.sqrt(r))
    return float(om) if om.ndim == 0 else om


def _hotspot_layout(h, words=None):
    return _layout([("flux", (h.nt,)), ("sx", (h.nt,)), ("sy", (h.nt,)), ("spectrogram", (h.nt, h.ne))],
                   [("on_disc", _rounded), ("used", _rounded), ("bad_angle", _rounded), (None, None)], words)


def hotspot_words(h):
    """Length of the buffer of kr_post_hotspot_dev_f64 / kr_reduce_hotspot_dev_f64: [flux | sx | sy (nt each) | spec (nt x ne) | on_disc | used | bad_angle | 0]."""
    return _hotspot_layout(h)


def hotspot_times(h):
    """The nt observer times T_k = t0 + k dt at which the spot is sampled."""
    return h.t0 + np.arange(h.nt) * h.dt


def hotspot_energies(h):
    """The centres of the ne energy bins of the spectrogram (geometric centres with log_e)."""
    i = np.arange(h.ne) + 0.5
    return h.e_min * np.float64(h.de) ** i if h.log_e else h.e_min + i * h.de


def hotspot_from_words(h, words):
    """The buffer of the hot-spot entry points as a dict: time (nt), flux, sx, sy, the centroids x = sx / flux and y = sy / flux (NaN where flux == 0),
    spectrogram (nt x ne) with `energy` (ne), and the tallies on_disc, used, bad_angle.  With several spots added into one buffer the tallies count
    every spot's pass."""
    out = _hotspot_layout(h, words)
    out["time"], out["energy"] = hotspot_times(h), hotspot_energies(h)
    with np.errstate(all="ignore"):
        lit = out["flux"] != 0
        out["x"] = np.where(lit, out["sx"] / np.where(lit, out["flux"], 1.0), np.nan)
        out["y"] = np.where(lit, out["sy"] / np.where(lit, out["flux"], 1.0), np.nan)
    return out


def reduce_hotspot(h, rays):
    """kr_reduce_hotspot_f64: the isotropic light curve of one spot from host ray records that carry their redshift and wrapped phi."""
    _rays_arg(rays, capi.RAY_F64)
    out = np.zeros(hotspot_words(h))
    capi.check(lib(), lib().kr_reduce_hotspot_f64(C.byref(h), _ptr(rays), len(rays), _ptr(out)), "kr_reduce_hotspot")
    return hotspot_from_words(h, out)


def _hotspot_stokes_layout(h, words=None):
    return _layout([(k, (h.nt,)) for k in ("flux", "sx", "sy", "q", "u")] + [("spectrogram", (h.nt, h.ne))],
                   [("on_disc", _rounded), ("used", _rounded), ("bad_pol", _rounded), (None, None)], words)


def hotspot_stokes_words(h):
    """Length of the buffer of kr_post_hotspot_stokes_dev_f64 / kr_reduce_hotspot_stokes_dev_f64:
    [flux | sx | sy | Q | U (nt each) | spec (nt x ne) | on_disc | used | bad_pol | 0]."""
    return _hotspot_stokes_layout(h)


def hotspot_stokes_from_words(h, words):
    """The buffer of the Stokes hot-spot entry points as a dict: what hotspot_from_words gives (without bad_angle) and q, u (nt: the Stokes sums on the
    plane's own x and y axes), pol_degree = sqrt(q^2 + u^2) / flux and pol_angle = atan2(u, q) / 2 in radians from the x axis towards the y axis (both
    NaN where flux == 0), and the tally bad_pol."""
    out = _hotspot_stokes_layout(h, words)
    out["time"], out["energy"] = hotspot_times(h), hotspot_energies(h)
    with np.errstate(all="ignore"):
        lit = out["flux"] != 0
        safe = np.where(lit, out["flux"], 1.0)
        out["x"] = np.where(lit, out["sx"] / safe, np.nan)
        out["y"] = np.where(lit, out["sy"] / safe, np.nan)
        out["pol_degree"] = np.where(lit, np.hypot(out["q"], out["u"]) / safe, np.nan)
        out["pol_angle"] = np.where(lit, 0.5 * np.arctan2(out["u"], out["q"]), np.nan)
    return out


def reduce_hotspot_stokes(spot, rays, spin, inc_deg, pol, limb=None):
    """kr_reduce_hotspot_stokes_f64: the light curve of one spot with its Stokes sums from host ray records of an image plane that carry their redshift
    and wrapped phi.  spin: the true spin (the a of the redshift pass with reverse = 1); inc_deg: the plane's inclination; pol, limb: as for
    stokes_image.  Keplerian gas (V = -1), projradius 0."""
    _rays_arg(rays, capi.RAY_F64)
    law, plaw = capi.limb_law(limb if limb is not None else "isotropic"), capi.pol_law(pol)
    out = np.zeros(hotspot_stokes_words(spot))
    capi.check(lib(), lib().kr_reduce_hotspot_stokes_f64(spin, -1.0, 1, 0, inc_deg, C.byref(spot), C.byref(law), C.byref(plaw), _ptr(rays), len(rays), _ptr(out)),
               "kr_reduce_hotspot_stokes")
    return hotspot_stokes_from_words(spot, out)


def hotspot_lightcurve(imageplane_spec, params, spots, limb=None, return_records=False, pol=None):
    """The light curve, centroid track and spectrogram of hot spots on the disc seen on an image plane, resident on the device from start to finish, as
    the kr_hotspot_lightcurve app runs it: ImagePlane ctor + redshift_start -> trace (`params` as for the image app: the stored, negated spin) ->
    redshift + range_phi + the first spot (kr_post_hotspot_dev_f64) -> every further spot on the records that pass left (kr_reduce_hotspot_dev_f64: those
    are isotropic, so several spots need limb=None) into the same buffer.  spots: a capi.HotSpot or a list of them on the same observer times and energy
    grid (anything else is refused; the line energies may differ); their outputs add.  Every spot is validated by the library before the plane is traced.
    Only the words are read back (and, with return_records, the final records: for tests).  Returns hotspot_from_words(...) plus "stats".  The sums are
    per image-plane pixel: multiply by dx dy / D^2 for a flux.
    pol: None, or a polarisation degree law as for stokes_image ((law, coeff), a name of capi.POL_LAWS or a capi.PolLaw): the Stokes light curves.  The
    first spot goes through kr_post_hotspot_stokes_dev_f64 at the plane's own inclination, every further one through kr_reduce_hotspot_stokes_dev_f64,
    which takes the limb law too: several spots may then share any limb law.  Returns hotspot_stokes_from_words(...) plus "stats": "q", "u",
    "pol_degree", "pol_angle" and "bad_pol" join the result (and "bad_angle" leaves it: bad-angle is a subset of bad-pol)."""
    spots = [spots] if isinstance(spots, capi.HotSpot) else list(spots)
    if not spots:
        raise KrError("hotspot_lightcurve: no spot")
    h = spots[0]

    def axes(s):
        return (s.nt, s.t0, s.dt, s.ne) + ((s.log_e, s.e_min, s.de) if s.ne > 0 else ())
    if any(axes(s) != axes(h) for s in spots):
        raise KrError("hotspot_lightcurve: the spots must share the observer times (nt, t0, dt) and the energy grid (ne, log_e, e_min, de): they add into one buffer")
    law = capi.limb_law(limb if limb is not None else "isotropic")
    if pol is not None:
        plaw, spin, inc = capi.pol_law(pol), -1 * imageplane_spec.spin, imageplane_spec.inc_deg

        def stokes_passes(L, dev, d_rays, n, d_out):
            capi.check(L, L.kr_post_hotspot_stokes_dev_f64(spin, -1.0, 1, 0, 0, -np.pi, np.pi, inc, C.byref(h), C.byref(law), C.byref(plaw), d_rays, n, d_out, None),
                       "kr_post_hotspot_stokes")
            for s in spots[1:]:
                capi.check(L, L.kr_reduce_hotspot_stokes_dev_f64(spin, -1.0, 1, 0, inc, C.byref(s), C.byref(law), C.byref(plaw), d_rays, n, d_out, None),
                           "kr_reduce_hotspot_stokes")

        words, stats, records = _imageplane_run("hotspot_lightcurve", imageplane_spec, params, hotspot_stokes_words(h), stokes_passes, return_records,
                                                before=lambda L, dev: stokes_passes(L, dev, None, 0, dev.zeros(8)))
        res = hotspot_stokes_from_words(h, words)
        res["stats"] = stats
        if return_records:
            res["records"] = records
        return res
    if len(spots) > 1 and law.law != 0:
        raise KrError("hotspot_lightcurve: several spots need the isotropic law (the further spots go through the reduce form)")
    def passes(L, dev, d_rays, n, d_out):
        capi.check(L, L.kr_post_hotspot_dev_f64(-1 * imageplane_spec.spin, -1.0, 1, 0, 0, -np.pi, np.pi, C.byref(h), C.byref(law), d_rays, n, d_out, None), "kr_post_hotspot")
        for s in spots[1:]:
            capi.check(L, L.kr_reduce_hotspot_dev_f64(C.byref(s), d_rays, n, d_out, None), "kr_reduce_hotspot")

    # the library's own refusals, before anything is traced: n = 0 validates the spots and the law and adds nothing (the buffer is not touched)
    words, stats, records = _imageplane_run("hotspot_lightcurve", imageplane_spec, params, hotspot_words(h), passes, return_records,
                                            before=lambda L, dev: passes(L, dev, None, 0, dev.zeros(8)))
    res = hotspot_from_words(h, words)
    res["stats"] = stats
    if return_records:
        res["records"] = records
    return res


def hotspot_text(res):
    """The file kr_hotspot_lightcurve writes for a result of hotspot_lightcurve(): three comment rows with the tallies ("# ON_DISC", "# USED",
    "# BAD_ANGLE"), one row per observer time: T flux x_c y_c, and, with a spectrogram, one block per observer time after a blank line each: a row
    T E_mid value per energy bin.  Every field setw(20), the numbers scientific with precision 8 (host/include/text_output.h).  A result that carries
    Stokes sums (hotspot_lightcurve(pol=...)): the third tally is "# BAD_POL" and the rows are T flux x_c y_c Q U."""
    stokes = "q" in res
    head = "".join("%20s%20d\n" % (f"# {k.upper()}", res[k]) for k in ("on_disc", "used", "bad_pol" if stokes else "bad_angle"))
    columns = [res[k] for k in (("time", "flux", "x", "y", "q", "u") if stokes else ("time", "flux", "x", "y"))]
    rows = "".join("".join(_path_field(float(v)) for v in row) + "\n" for row in zip(*columns))
    blocks = "".join("\n" + "".join(_path_field(float(t)) + _path_field(float(e)) + _path_field(float(v)) + "\n" for e, v in zip(res["energy"], row))
                     for t, row in zip(res["time"], res["spectrogram"])) if len(res["energy"]) else ""
    return head + rows + blocks
