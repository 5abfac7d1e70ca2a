"""TEST INFRASTRUCTURE: the per-pixel rules of the reference's caustic_sourceplane program (src/caustic/caustic_sourceplane.cpp:68-73, :180-232,
:264-305) and caustic_plane program (src/caustic/caustic_plane.cpp:180-189, :207-299, :315-392; ray_destination.h:195-203) restated in numpy over
ray records, in the manner of tests/caustic_rules.py.  tests/test_source_caustic_rules.py pins this restatement to the compiled reference's own FITS
output before tests/test_gpu_source_caustic.py lets it judge the device kernels.

Planes are (nx, ny) arrays indexed [ix, iy] like the programs' Array2D.  sin / cos / atan2 are the C library's, one call per element (math.*)."""
import math

import numpy as np

from caustic_rules import SENTINEL, bits_equal, det_bound, read_par, plane_geometry as _disc_geometry, fits_planes as _disc_fits_planes, golden  # noqa: F401

PLANES = {"sphere": ("DET_J", "SIGN_J", "ORDER", "ESCAPED", "THETA_S", "PHI_S", "RDOT_FLIPS", "EQUAT_CROSS"),
          "plane": ("DET_J", "SIGN_J", "ORDER", "HIT_PLANE", "X_S", "Y_S", "RDOT_FLIPS", "EQUAT_CROSS")}
HIT = {"sphere": "ESCAPED", "plane": "HIT_PLANE"}
COORDS = {"sphere": ("THETA_S", "PHI_S"), "plane": ("X_S", "Y_S")}
COUNT_CARDS = {"sphere": ("N_ESC", "N_CAP", "N_SLIM"), "plane": ("N_HIT", "N_CAP", "N_SLIM")}
STATUS_DEST, STATUS_HORIZON, STATUS_RLIM, STATUS_STEPLIM = 1, 2, 4, 8

_sin, _cos, _atan2 = np.vectorize(math.sin, otypes=[float]), np.vectorize(math.cos, otypes=[float]), np.vectorize(math.atan2, otypes=[float])


def plane_geometry(par, kind):
    """The numbers caustic_sourceplane.cpp:89-137 / caustic_plane.cpp:79-137 derive from the parameter file."""
    full = dict(par, r_disc=0)                       # (these programs have no disc; their axis defaults are -20 .. 20, y as x)
    full.setdefault("x0", "-20")
    full.setdefault("xmax", "20")
    full.setdefault("y0", full["x0"])
    full.setdefault("ymax", full["xmax"])
    g = _disc_geometry(full)
    del g["r_disc"]
    g["steplim"] = int(par.get("steplim", -1))
    if kind == "sphere":
        g["r_lim"] = float(par.get("r_lim", 1.5 * g["dist"]))
        g["eps_frac"] = 0.0
    else:
        g["z_s"] = float(par.get("z_s", g["dist"]))
        g["r_max"] = float(par.get("r_max", 4.0 * g["z_s"]))
        g["incl_rad"] = g["incl"] * math.pi / 180.0
    return g


def fits_planes(path, kind):
    """The eight planes of a caustic_sourceplane / caustic_plane FITS file as [ix, iy] arrays, and the primary header."""
    import fits_lite
    hdus = fits_lite.read(path)
    assert [h["name"] for h in hdus] == ["PRIMARY"] + list(PLANES[kind]), [h["name"] for h in hdus]
    return {h["name"]: np.asarray(h["data"], dtype=np.float64).T.copy() for h in hdus[1:]}, hdus[0]["header"]


def _sign(det):
    return np.where(det > 0, 1.0, np.where(det < 0, -1.0, 0.0))


def sphere_hit(r):
    """escaped, caustic_sourceplane.cpp:191"""
    return (r["steps"] > 0) & ((r["status"] & STATUS_RLIM) != 0)


def plane_hit(r):
    """valid_hit, caustic_plane.cpp:187-189"""
    return (r["steps"] > 0) & ((r["status"] & STATUS_DEST) != 0)


def sphere_coords(r):
    """(theta_s, phi_s, order), caustic_sourceplane.cpp:202-214; records with a non-finite phi give NaN"""
    ok = np.isfinite(r["phi"])
    phi = np.where(ok, r["phi"], 0.0)
    ps = np.where(ok, _atan2(_sin(phi), _cos(phi)), np.nan)
    phi_order = np.floor(np.abs(phi) / math.pi).astype(np.int64)
    return r["theta"].copy(), ps, np.where(phi_order > 0, phi_order - 1, 0)


def plane_coords(r, incl, phi0):
    """(x_s, y_s, order): FlatPlaneDestination::source_coords (ray_destination.h:195-203) in its association, and plane_order (caustic_plane.cpp:180-184)"""
    ok = np.isfinite(r["phi"]) & np.isfinite(r["theta"])
    phi, theta = np.where(ok, r["phi"], 0.0), np.where(ok, r["theta"], 0.0)
    st, ct, sp, cp = _sin(theta), _cos(theta), _sin(phi), _cos(phi)
    si, ci, s0, c0 = math.sin(incl), math.cos(incl), math.sin(phi0), math.cos(phi0)
    X, Y, Z = r["r"] * st * cp, r["r"] * st * sp, r["r"] * ct
    xs = -X * s0 + Y * c0
    ys = -X * ci * c0 - Y * ci * s0 + Z * si
    order = np.maximum((np.abs(phi) / (2 * math.pi)).astype(np.int64), r["rdot_flips"] // 2)
    return np.where(ok, xs, np.nan), np.where(ok, ys, np.nan), order


def centre_planes(c, kind, incl=0.0, phi0=0.0):
    """the six planes every mode takes from the ray through the pixel, and the three counts (caustic_sourceplane.cpp:180-232, caustic_plane.cpp:207-241)"""
    if kind == "sphere":
        hit = sphere_hit(c)
        u, v, order = sphere_coords(c)
    else:
        hit = plane_hit(c)
        u, v, order = plane_coords(c, incl, phi0)
    ku, kv = COORDS[kind]
    maps = {HIT[kind]: hit.astype(float), ku: np.where(hit, u, np.nan), kv: np.where(hit, v, np.nan), "ORDER": np.where(hit, order, -1).astype(float),
            "RDOT_FLIPS": c["rdot_flips"].astype(float), "EQUAT_CROSS": c["equatorial_crossings"].astype(float)}
    counts = {"hit": int(hit.sum()), "captured": int((~hit & ((c["status"] & STATUS_HORIZON) != 0)).sum()),
              "steplim": int(((c["steps"] <= 0) | ((c["status"] & STATUS_STEPLIM) != 0)).sum())}
    return maps, counts


def wrap_dphi(d):
    """caustic_sourceplane.cpp:68-73 on differences of two angles in [-pi, pi]: each loop runs at most once"""
    d = np.where(d > math.pi, d - 2 * math.pi, d)
    return np.where(d < -math.pi, d + 2 * math.pi, d)


def grid_maps(rays, nx, ny, kind, dx, dy, incl=0.0, phi0=0.0):
    """Grid-neighbour mode: rays[ix ny + iy] (caustic_sourceplane.cpp:180-305, caustic_plane.cpp:315-392).  Returns (planes, counts, G, raw): G = the
    largest |derivative| of each pixel (NaN where no determinant was formed); raw = for the sphere, per pixel the |raw phi difference| of the two
    neighbour pairs that lies closest to pi (NaN where no determinant was formed), else None."""
    c = rays[:nx * ny].reshape(nx, ny)
    maps, counts = centre_planes(c, kind, incl, phi0)
    ku, kv = COORDS[kind]
    hit, order, U, V = maps[HIT[kind]] != 0, maps["ORDER"], maps[ku], maps[kv]
    det = np.full((nx, ny), np.nan)
    sign = np.zeros((nx, ny))
    G = np.full((nx, ny), np.nan)
    raw = np.full((nx, ny), np.nan) if kind == "sphere" else None
    if nx > 2 and ny > 2:
        i = (slice(1, -1), slice(1, -1))
        e, w, n, s = (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1)), (slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2))
        allhit = hit[i] & hit[e] & hit[w] & hit[n] & hit[s]
        match = (order[e] == order[i]) & (order[w] == order[i]) & (order[n] == order[i]) & (order[s] == order[i])
        with np.errstate(invalid="ignore"):
            dvx, dvy = V[e] - V[w], V[n] - V[s]
            if kind == "sphere":
                near = np.minimum(np.abs(np.abs(dvx) - math.pi), np.abs(np.abs(dvy) - math.pi))
                dvx, dvy = wrap_dphi(dvx), wrap_dphi(dvy)
            a11, a12, a21, a22 = (U[e] - U[w]) / (2 * dx), (U[n] - U[s]) / (2 * dy), dvx / (2 * dx), dvy / (2 * dy)
            d = a11 * a22 - a12 * a21
        ok = allhit & match
        det[i] = np.where(ok, d, np.where(allhit, SENTINEL, np.nan))
        sign[i] = np.where(ok, _sign(d), 0.0)
        G[i] = np.where(ok, np.maximum.reduce([np.abs(a11), np.abs(a12), np.abs(a21), np.abs(a22)]), np.nan)
        if kind == "sphere":
            raw[i] = np.where(ok, near, np.nan)
    maps["DET_J"], maps["SIGN_J"] = det, sign
    return maps, counts, G, raw


def bundle_maps(rays, nx, ny, eps_x, eps_y, incl, phi0):
    """Plane kind, bundle mode: rays[(ix ny + iy) 5 + m], m = centre, east, west, north, south (caustic_plane.cpp:207-299).  Returns (planes, counts, G)."""
    B = rays[:5 * nx * ny].reshape(nx, ny, 5)
    c, sat = B[:, :, 0], [B[:, :, m] for m in (1, 2, 3, 4)]
    maps, counts = centre_planes(c, "plane", incl, phi0)
    allhit = maps["HIT_PLANE"] != 0
    match = np.ones((nx, ny), bool)
    for s in sat:
        allhit = allhit & plane_hit(s)
        with np.errstate(invalid="ignore"):
            match &= (s["rdot_flips"] == c["rdot_flips"]) & (np.abs(s["phi"] - c["phi"]) < math.pi / 2)
    (xe, ye, _), (xw, yw, _), (xn, yn, _), (xs, ys, _) = [plane_coords(s, incl, phi0) for s in sat]
    with np.errstate(invalid="ignore"):
        a11, a12, a21, a22 = (xe - xw) / (2 * eps_x), (xn - xs) / (2 * eps_y), (ye - yw) / (2 * eps_x), (yn - ys) / (2 * eps_y)
        d = a11 * a22 - a12 * a21
    det = np.full((nx, ny), np.nan)
    sign = np.zeros((nx, ny))
    det[allhit & ~match] = SENTINEL
    ok = allhit & match
    det[ok] = d[ok]
    sign[ok] = _sign(d[ok])
    maps["DET_J"], maps["SIGN_J"] = det, sign
    G = np.where(ok, np.maximum.reduce([np.abs(a11), np.abs(a12), np.abs(a21), np.abs(a22)]), np.nan)
    return maps, counts, G
