"""TEST INFRASTRUCTURE: the per-pixel rules of the reference's caustic_discplane program (src/caustic/caustic_discplane.cpp:170-202, :219-334,
:403-493) restated in numpy over ray records, in the manner of tests/line_rules.py.  tests/test_caustic_rules.py pins this restatement to the
compiled reference's own FITS output before tests/test_gpu_caustic.py lets it judge the device kernels.

Planes are (nx, ny) arrays indexed [ix, iy] like the program's Array2D (tests/fits_lite.read returns FITS images as [iy][ix]: use fits_planes()).
sin / cos / atan2 are the C library's, one call per element (math.*), like the program's."""
import math
import os

import numpy as np

PLANES = ("DET_J", "SIGN_J", "ORDER", "HIT", "RADIUS", "PHI", "X_DISC", "Y_DISC", "REDSHIFT")
SENTINEL = 1e30

_sin, _cos, _atan2 = np.vectorize(math.sin, otypes=[float]), np.vectorize(math.cos, otypes=[float]), np.vectorize(math.atan2, otypes=[float])


def read_par(path):
    """key = value lines of a parameter file (comments from '#')."""
    out = {}
    for line in open(path):
        line = line.split("#", 1)[0].strip()
        if "=" in line:
            k, v = line.split("=", 1)
            out[k.strip()] = v.strip()
    return out


def plane_geometry(par):
    """The numbers caustic_discplane.cpp:84-130 derives from the parameter file."""
    g = {k: float(par[k]) for k in ("dist", "incl", "spin", "r_disc", "x0", "xmax", "y0", "ymax")}
    g["phi0"] = float(par.get("plane_phi0", 0))
    g["Nx"], g["Ny"] = int(par["Nx"]), int(par.get("Ny", par["Nx"]))
    g["dx"], g["dy"] = (g["xmax"] - g["x0"]) / g["Nx"], (g["ymax"] - g["y0"]) / g["Ny"]
    g["nx"], g["ny"] = g["Nx"] + 1, g["Ny"] + 1
    g["eps_frac"] = float(par.get("bundle_eps_frac", 0.01))
    g["integrator"] = par.get("integrator", "rk45")
    g["rk45_tol"] = float(par.get("rk45_tol", 1e-8))
    g["precision"] = float(par.get("precision", 100))
    return g


def valid_hit(r, r_isco, r_disc):
    """:177-182"""
    with np.errstate(invalid="ignore"):
        return (r["steps"] > 0) & (r["r"] >= r_isco) & (r["r"] < r_disc) & (r["redshift"] > 0)


def disc_xy(r):
    """:170-174 -> (x_disc, y_disc, phi_s); records with a non-finite phi give NaN (they are never valid hits)"""
    ok = np.isfinite(r["phi"])
    phi = np.where(ok, r["phi"], 0.0)
    ps = _atan2(_sin(phi), _cos(phi))
    ps = np.where(ok, ps, np.nan)
    safe = np.where(ok, ps, 0.0)
    return np.where(ok, r["r"] * _cos(safe), np.nan), np.where(ok, r["r"] * _sin(safe), np.nan), ps


def diagnostics(c, r_isco, r_disc):
    """:255-276 over the centre rays -> dict of the five failure counts"""
    from raytrace_cpu_amd import capi
    with np.errstate(invalid="ignore"):
        oor = (c["steps"] > 0) & ((c["r"] < r_isco) | (c["r"] >= r_disc) | (c["redshift"] <= 0))
    rest = ~oor & ((c["steps"] <= 0) | ((c["status"] & capi.STATUS_DEST) == 0))
    hz = rest & ((c["status"] & capi.STATUS_HORIZON) != 0)
    rl = rest & ~hz & ((c["status"] & capi.STATUS_RLIM) != 0)
    sl = rest & ~hz & ~rl & ((c["status"] & capi.STATUS_STEPLIM) != 0)
    return {"horizon": int(hz.sum()), "rlim": int(rl.sum()), "steplim": int(sl.sum()), "out_of_range": int(oor.sum()), "other": int((rest & ~hz & ~rl & ~sl).sum())}


def _sign(det):
    return np.where(det > 0, 1.0, np.where(det < 0, -1.0, 0.0))


def centre_planes(c, r_isco, r_disc):
    """:219-251 (and :351-380): the seven planes every mode takes from the ray through the pixel"""
    hit = valid_hit(c, r_isco, r_disc)
    x, y, ps = disc_xy(c)
    phi = np.where(np.isfinite(c["phi"]), c["phi"], 0.0)
    order = np.maximum((np.abs(phi) / (2 * math.pi)).astype(np.int64), c["rdot_flips"] // 2)        # disc_order, :198-202 (rdot_flips >= 0)
    return {"HIT": hit.astype(float), "RADIUS": np.where(hit, c["r"], 0.0), "PHI": np.where(hit, ps, 0.0), "X_DISC": np.where(hit, x, 0.0),
            "Y_DISC": np.where(hit, y, 0.0), "ORDER": np.where(hit, order, -1).astype(float), "REDSHIFT": np.where(hit, c["redshift"], 0.0)}


def wrap_dphi(d):
    """caustic_sourceplane.cpp:68-73 on differences of two angles in [-pi, pi]: each loop runs at most once"""
    d = np.where(d > math.pi, d - 2 * math.pi, d)
    return np.where(d < -math.pi, d + 2 * math.pi, d)


def satellite_jacobian(c, sat, coords, eps_x, eps_y):
    """The Jacobian of a pixel from its four satellites (caustic_discplane.cpp:279-334, caustic_plane.cpp:249-299): c = the (nx, ny) centre rays,
    sat = [east, west, north, south], coords(records) -> (hit, u, v).  Returns (det, sign, G): G = the largest |derivative| of each pixel (NaN where
    no determinant was formed)."""
    allhit = coords(c)[0]
    match = np.ones(c.shape, bool)
    for s in sat:
        with np.errstate(invalid="ignore"):
            match &= (s["rdot_flips"] == c["rdot_flips"]) & (np.abs(s["phi"] - c["phi"]) < math.pi / 2)
    (he, ue, ve), (hw, uw, vw), (hn, un, vn), (hs, us, vs) = [coords(s) for s in sat]
    allhit = allhit & he & hw & hn & hs
    with np.errstate(invalid="ignore"):
        a11, a12, a21, a22 = (ue - uw) / (2 * eps_x), (un - us) / (2 * eps_y), (ve - vw) / (2 * eps_x), (vn - vs) / (2 * eps_y)
        d = a11 * a22 - a12 * a21
    ok = allhit & match
    det = np.where(ok, d, np.where(allhit, SENTINEL, np.nan))
    G = np.where(ok, np.maximum.reduce([np.abs(a11), np.abs(a12), np.abs(a21), np.abs(a22)]), np.nan)
    return det, np.where(ok, _sign(d), 0.0), G


def neighbour_jacobian(hit, order, U, V, dx, dy, wrap=False):
    """The Jacobian of a pixel from its four grid neighbours (caustic_discplane.cpp:403-439, caustic_sourceplane.cpp:264-305, caustic_plane.cpp:357-392)
    over the (nx, ny) planes; wrap: V is an angle, its differences go through wrap_dphi.  Returns (det, sign, G, raw): G as satellite_jacobian's;
    raw = with wrap, per pixel the |raw V difference| of the two neighbour pairs that lies closest to pi (NaN where no determinant was formed), else None."""
    nx, ny = hit.shape
    det = np.full((nx, ny), np.nan)
    sign = np.zeros((nx, ny))
    G = np.full((nx, ny), np.nan)
    raw = np.full((nx, ny), np.nan) if wrap else None
    if nx > 2 and ny > 2:
        i = (slice(1, -1), slice(1, -1))
        e, w, n, s = (slice(2, None), slice(1, -1)), (slice(0, -2), slice(1, -1)), (slice(1, -1), slice(2, None)), (slice(1, -1), slice(0, -2))
        allhit = hit[i] & hit[e] & hit[w] & hit[n] & hit[s]
        match = (order[e] == order[i]) & (order[w] == order[i]) & (order[n] == order[i]) & (order[s] == order[i])
        with np.errstate(invalid="ignore"):
            dvx, dvy = V[e] - V[w], V[n] - V[s]
            if wrap:
                near = np.minimum(np.abs(np.abs(dvx) - math.pi), np.abs(np.abs(dvy) - math.pi))
                dvx, dvy = wrap_dphi(dvx), wrap_dphi(dvy)
            a11, a12, a21, a22 = (U[e] - U[w]) / (2 * dx), (U[n] - U[s]) / (2 * dy), dvx / (2 * dx), dvy / (2 * dy)
            d = a11 * a22 - a12 * a21
        ok = allhit & match
        det[i] = np.where(ok, d, np.where(allhit, SENTINEL, np.nan))
        sign[i] = np.where(ok, _sign(d), 0.0)
        G[i] = np.where(ok, np.maximum.reduce([np.abs(a11), np.abs(a12), np.abs(a21), np.abs(a22)]), np.nan)
        if wrap:
            raw[i] = np.where(ok, near, np.nan)
    return det, sign, G, raw


def bundle_maps(rays, nx, ny, r_isco, r_disc, eps_x, eps_y):
    """Bundle mode, before suppression: rays[(ix ny + iy) 5 + m], m = centre, east, west, north, south (:219-334).
    Returns (planes, counts, G): G = the largest |derivative| of each pixel (NaN where no determinant was formed)."""
    B = rays[:5 * nx * ny].reshape(nx, ny, 5)
    c = B[:, :, 0]
    maps = centre_planes(c, r_isco, r_disc)
    maps["DET_J"], maps["SIGN_J"], G = satellite_jacobian(c, [B[:, :, m] for m in (1, 2, 3, 4)], lambda r: (valid_hit(r, r_isco, r_disc),) + disc_xy(r)[:2], eps_x, eps_y)
    return maps, dict(diagnostics(c, r_isco, r_disc), disc_count=int((maps["HIT"] != 0).sum())), G


def grid_maps(rays, nx, ny, r_isco, r_disc, dx, dy):
    """Grid-neighbour mode, before suppression: rays[ix ny + iy] (:349-439).  Returns (planes, counts, G)."""
    c = rays[:nx * ny].reshape(nx, ny)
    maps = centre_planes(c, r_isco, r_disc)
    maps["DET_J"], maps["SIGN_J"], G, _ = neighbour_jacobian(maps["HIT"] != 0, maps["ORDER"], maps["X_DISC"], maps["Y_DISC"], dx, dy)
    return maps, dict(diagnostics(c, r_isco, r_disc), disc_count=int((maps["HIT"] != 0).sum())), G


def suppress(maps):
    """:455-493, in place on maps["DET_J"] / maps["SIGN_J"], over a snapshot of SIGN_J.  Returns the number of pixels suppressed."""
    sc = maps["SIGN_J"].copy()
    nx, ny = sc.shape
    same, opp = np.zeros((nx, ny), int), np.zeros((nx, ny), int)
    pad = np.zeros((nx + 2, ny + 2))
    pad[1:-1, 1:-1] = sc
    for sx, sy in ((0, 1), (2, 1), (1, 0), (1, 2)):
        sn = pad[sx:sx + nx, sy:sy + ny]
        prod = sn * sc
        same += (prod > 0)
        opp += (sn != 0) & (sc != 0) & ~(prod > 0)
    hitlist = (sc != 0) & (opp > same) & (opp >= 2)
    maps["DET_J"][hitlist] = SENTINEL
    maps["SIGN_J"][hitlist] = 0.0
    return int(hitlist.sum())


def fits_planes(path):
    """The nine planes of a caustic_discplane FITS file as [ix, iy] arrays, and the primary header."""
    import fits_lite
    hdus = fits_lite.read(path)
    assert [h["name"] for h in hdus] == ["PRIMARY"] + list(PLANES), [h["name"] for h in hdus]
    return {h["name"]: np.asarray(h["data"], dtype=np.float64).T.copy() for h in hdus[1:]}, hdus[0]["header"]


def bits_equal(a, b):
    """elementwise: same bits, or both NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def det_bound(c, eps, G):
    """First-order propagation of an absolute error c on each X_DISC / Y_DISC value through the central differences over 2 eps and the 2 x 2
    determinant: each derivative moves by <= c / eps, the determinant by <= 2 * 2 * (c / eps) * G."""
    return 4 * (c / eps) * G


def golden(name):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "apps", name)
