"""numpy restatement of the emission-line binning rules of include/kr_trace.h (kr_line_bins), the reference notebook's line
(python/line_from_image.ipynb) and the comparison rule of the line tests.  TEST INFRASTRUCTURE: nothing here runs in the product path."""
import numpy as np

from raytrace_cpu_amd import capi


def powerlaw3(r, q1, rb1, q2, rb2, q3):
    """imageplane_disc_image.cpp:20-28, elementwise."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(r < rb1, r ** (-1 * q1),
                        np.where(r < rb2, rb1 ** (q2 - q1) * r ** (-1 * q2), rb1 ** (q2 - q1) * rb2 ** (q3 - q2) * r ** (-1 * q3)))


def has_time_axis(b):
    return not (b.nt == 1 and b.dt <= 0)


def table_of(b):
    """(emis, time or None) of the bins' host table, or (None, None)."""
    if not b.table_emis:
        return None, None
    emis = np.ctypeslib.as_array(b.table_emis, shape=(b.table_nr,)).copy()
    time = np.ctypeslib.as_array(b.table_time, shape=(b.table_nr,)).copy() if b.table_time else None
    return emis, time


def items(b, r, x, t, pixel=False):
    """Per item (ray or pixel) that passed the filter: (E, w, tau, binnable).  x = g for rays, the mean 1/g for pixels."""
    r, x, t = (np.asarray(a, dtype=np.float64) for a in (r, x, t))
    temis, ttime = table_of(b)
    ok = np.ones(r.shape, dtype=bool)
    tt = np.zeros_like(r)
    with np.errstate(all="ignore"):
        if temis is not None:
            fi = np.log(r / b.table_r_min) / np.log(b.table_dr) if b.table_logbin else (r - b.table_r_min) / b.table_dr
            inside = (fi > -1) & (fi < b.table_nr)
            ir = np.where(inside, np.trunc(np.where(inside, fi, 0)), 0).astype(np.int64)
            emis = np.where(inside, temis[ir], np.nan)
            ok &= inside & np.isfinite(emis)
            if ttime is not None:
                tt = np.where(inside, ttime[ir], 0.0)
        else:
            emis = powerlaw3(r, b.q1, b.rb1, b.q2, b.rb2, b.q3)
        if pixel:
            E = b.line_energy * x
            w = emis * np.power(x, b.g_index)
        else:
            E = b.line_energy / x
            w = emis * np.power(x, -1 * b.g_index)
        tau = t + tt - b.t0
    return E, w, tau, ok


def bin_items(b, E, w, tau, ok, on_disc):
    """The bin rules: returns the dict of api.line_from_words (count / flux of shape (nt, ne), on_disc, binned)."""
    ne, nt = b.ne, b.nt
    with np.errstate(all="ignore"):
        fe = np.log(E / b.e_min) / np.log(b.de) if b.log_e else (E - b.e_min) / b.de
        keep = ok & (fe >= 0) & (fe < ne)
        if has_time_axis(b):
            ft = tau / b.dt
            keep &= (ft >= 0) & (ft < nt)
            j = np.where(keep, ft, 0).astype(np.int64)
        else:
            j = np.zeros(E.shape, dtype=np.int64)
        i = np.where(keep, fe, 0).astype(np.int64)
    k = j[keep] * ne + i[keep]
    count = np.bincount(k, minlength=nt * ne).astype(np.float64)
    flux = np.bincount(k, weights=w[keep], minlength=nt * ne)
    return {"count": count.reshape(nt, ne), "flux": flux.reshape(nt, ne), "on_disc": int(on_disc), "binned": int(keep.sum())}


def disc_filter(b, rays):
    """steps > 0, z = r cos(theta) < 1e-2, r_isco <= r < r_disc, g > 0 (imageplane_disc_image.cpp:127-128 without the pixel range)."""
    r, g = rays["r"], rays["redshift"]
    with np.errstate(invalid="ignore"):
        return (rays["steps"] > 0) & (r * np.cos(rays["theta"]) < 1e-2) & (r >= b.r_isco) & (r < b.r_disc) & (g > 0)


def line_from_rays(b, rays):
    """kr_reduce_line_f64 / kr_post_line_dev_f64 in numpy, on records after redshift(-1, reverse=1)."""
    m = disc_filter(b, rays)
    E, w, tau, ok = items(b, rays["r"][m], rays["redshift"][m], rays["t"][m])
    return bin_items(b, E, w, tau, ok, m.sum())


def line_from_means(b, nrays, enshift, r, t):
    """kr_line_from_image_dev_f64 in numpy, from per-pixel MEANS (enshift = mean 1/g); pixels with nrays > 0 count."""
    m = np.asarray(nrays) > 0
    E, w, tau, ok = items(b, np.asarray(r)[m], np.asarray(enshift)[m], np.asarray(t)[m], pixel=True)
    return bin_items(b, E, w, tau, ok, m.sum())


def line_from_fits(b, path):
    """The per-pixel line of an imageplane_disc_image FITS file: ENSHIFT, RADIUS, TIME are per-pixel means, NaN where no ray arrived."""
    import fits_lite
    h = {x["name"]: x["data"] for x in fits_lite.read(path)}
    en, r, t = h["ENSHIFT"].ravel(), h["RADIUS"].ravel(), h["TIME"].ravel()
    return line_from_means(b, np.isfinite(en).astype(np.int64), en, r, t)


def notebook_line(path, line_en, bin_edges, q1, rbreak, q2):
    """python/line_from_image.ipynb as written: broken power law (r <= rbreak), flux = emis enshift^3, NaN -> 0, sum by energy
    (binned_statistic(..., 'sum') == np.histogram with weights: half-open bins, the last one closed)."""
    import fits_lite
    h = {x["name"]: x["data"] for x in fits_lite.read(path)}
    enshift = np.array(h["ENSHIFT"], dtype=np.float64)
    disc_r = np.array(h["RADIUS"], dtype=np.float64)
    enshift[np.isnan(enshift)] = 0
    pl = np.zeros_like(disc_r)
    with np.errstate(invalid="ignore"):
        lo = disc_r <= rbreak
        hi = disc_r > rbreak
    pl[lo] = disc_r[lo] ** -q1
    pl[hi] = rbreak ** (q2 - q1) * disc_r[hi] ** -q2
    disc_flux = pl * enshift ** 3
    disc_flux[np.isnan(disc_flux)] = 0
    line, _ = np.histogram(line_en * enshift.flatten(), bins=bin_edges, weights=disc_flux.flatten())
    count, _ = np.histogram(line_en * enshift.flatten(), bins=bin_edges)
    return line, count


def read_emissivity_dat(path):
    """A 7-column emissivity table (r, area, rays, flux, emis, redshift, time): (r_min, edge ratio, emis, time), as kr_line_profile reads it."""
    a = np.loadtxt(path)
    r = a[:, 0]
    dr = np.exp(np.log(r[-1] / r[0]) / (len(r) - 1))
    assert np.all(np.abs(r / (r[0] * dr ** np.arange(len(r))) - 1) <= 1e-7), "r column is not log-spaced"
    return r[0], dr, a[:, 4].copy(), a[:, 6].copy()


def bins(**kw):
    return capi.line_bins(**kw)


def compare_line(got, want, rtol=1e-6, slack=1, max_excluded=None):
    """The rule of parity.compare_bins on the line's keys: counts within `slack` per bin, flux within rtol on bins whose counts agree,
    and at most max_excluded (default: 2 % of the non-empty bins, at least 2) non-empty bins left out of the flux check.
    Returns (problems, margins): problems empty = pass; margins = {"worst_flux_rel", "bins_excluded", "allowed", "max_count_diff"}."""
    problems = []
    gc, wc = np.asarray(got["count"]).ravel(), np.asarray(want["count"]).ravel()
    dc = np.abs(gc - wc)
    if (dc > slack).any():
        problems.append(("count", float(dc.max()), int(np.argmax(dc))))
    same = dc == 0
    nonempty = int((wc > 0).sum())
    excluded = int((~same & (wc > 0)).sum())
    bound = max(2, nonempty // 50) if max_excluded is None else max_excluded
    if excluded > bound:
        problems.append(("excluded_bins", excluded, bound))
    g, w = np.asarray(got["flux"]).ravel()[same], np.asarray(want["flux"]).ravel()[same]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(g == w, 0.0, np.abs(g - w) / np.maximum(np.abs(w), 1e-300))
    worst = float(rel.max()) if rel.size else 0.0
    if worst > rtol:
        problems.append(("flux", worst, int(np.argmax(rel))))
    return problems, {"worst_flux_rel": worst, "bins_excluded": excluded, "allowed": bound, "max_count_diff": float(dc.max()) if dc.size else 0.0}
