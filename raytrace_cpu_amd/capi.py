"""ctypes mirror of include/kr_trace.h (struct layouts, constants, prototypes).

Pure interface definitions: nothing here computes.  `load()` opens the HIP shared library
(raytrace_cpu_amd/csrc/libkrtrace.so) and fails loudly when it is missing -- there is no CPU
fallback in the product path.
"""
import ctypes as C
import os

import numpy as np

ABI_VERSION = 16

KR_OK, KR_EINVAL, KR_ENODEVICE, KR_EHIP, KR_ENOMEM = 0, -1, -2, -3, -4
EULER, RK4, RK45 = 0, 1, 2
STOP_THETA, STOP_FLATDISC, STOP_DISC_ISCO, STOP_FLATPLANE, STOP_THICKDISC = 0, 1, 2, 3, 4
STATUS_DEST, STATUS_HORIZON, STATUS_RLIM, STATUS_STEPLIM = 1, 2, 4, 8
STATUS_ERGO, STATUS_NEG_ENERGY, STATUS_NAN = 16, 32, 64
STEPLIM, RK45_STEPLIM, MIN_STEP = 10_000_000, 100_000, 1e-3
FLAG_FAST_MATH = 1
FLAG_HYBRID = 2
FLAG_RK45_ITERATE_ALL = 4

# the value of V that selects the disc flow "Keplerian, plunging inside the ISCO" in the passes that take it (KR_V_PLUNGE, include/kr_trace.h)
V_PLUNGE = -2.0

# Ray<double> / Ray<float>  (reference src/raytracer/raytracer.h:65-78)
_F64 = [(n, "<f8") for n in ("t", "r", "theta", "phi", "pt", "pr", "ptheta", "pphi", "k", "h", "Q", "emit", "redshift")]
_I32 = [(n, "<i4") for n in ("steps", "status", "rdot_sign", "thetadot_sign", "rdot_flips", "equatorial_crossings")]
RAY_F64 = np.dtype(_F64 + _I32 + [("alpha", "<f8"), ("beta", "<f8")], align=True)
RAY_F32 = np.dtype([(n, "<f4") for n, _ in _F64] + _I32 + [("alpha", "<f4"), ("beta", "<f4")], align=True)
assert RAY_F64.itemsize == 144 and RAY_F32.itemsize == 84


class Params(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("spin", "horizon", "precision", "theta_precision", "max_tstep",
                                          "maxtstep_rlim", "max_phistep", "rk45_tol", "r_max", "theta_max")] + \
               [("stop_params", C.c_double * 4)] + \
               [(n, C.c_int32) for n in ("integrator", "stop_kind", "steplim", "flags")]


class Stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("rays_total", "rays_traced", "steps_total", "rk45_attempts", "rk45_rejects")] + \
               [(n, C.c_double) for n in ("kernel_ms", "h2d_ms", "d2h_ms")] + [("rays_strict_side", C.c_int64), ("rk45_stationary_steps", C.c_int64), ("rk45_extrapolated_steps", C.c_int64)] + \
               [("strict_side_ms", C.c_double), ("main_ms", C.c_double), ("longest_ray_steps", C.c_int64), ("longest_ray_steps_strict_side", C.c_int64),
                ("steps_strict_side", C.c_int64), ("rk45_evaluated_strict_side", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PointSourceSpec(C.Structure):
    _fields_ = [("pos", C.c_double * 4)] + \
               [(n, C.c_double) for n in ("V", "spin", "tol", "dcosalpha", "dbeta", "cosalpha0", "cosalphamax",
                                          "beta0", "betamax", "E")]


class ImagePlaneSpec(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("dist", "inc_deg", "x0", "xmax", "dx", "y0", "ymax", "dy", "spin", "phi0",
                                          "precision")]


class EmisBins(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("r_min", "dr", "r_isco", "gamma", "spin", "num_primary_rays")] + \
               [("nr", C.c_int32), ("logbin", C.c_int32)]


class ImageBins(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("x0", "y0", "img_dx", "img_dy", "r_isco", "r_disc", "q1", "rb1", "q2", "rb2", "q3")] + \
               [(n, C.c_int32) for n in ("img_nx", "img_ny", "flip_image", "pad")]


class ReturnBins(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("r_isco", "r_disc", "r_esc", "source_r", "source_phi")] + \
               [(n, C.c_int32) for n in ("plane_iso", "limb", "weight_norm", "pad")]


class ReturnMap(C.Structure):
    """kr_return_map: the landing map of the returning radiation -- kr_return_bins (cls) plus the landing-radius bins (include/kr_trace.h has the
    per-ray rule)."""
    _fields_ = [("cls", ReturnBins), ("r_min", C.c_double), ("dr", C.c_double), ("gamma", C.c_double), ("nr", C.c_int32), ("logbin", C.c_int32)]


class HealpixSource(C.Structure):
    """kr_healpix_source: a point source whose sky is sampled by HEALPix pixels, orbiting (motion 0) or moving radially (motion 1)
    (include/kr_trace.h has the geometry, the ray rule and what is refused)."""
    _fields_ = [("pos", C.c_double * 4)] + [(n, C.c_double) for n in ("V", "spin", "E")] + \
               [(n, C.c_int32) for n in ("order", "motion", "basis", "rays_per_pixel", "unit_center", "disc_source")]


class HealpixMap(C.Structure):
    """kr_healpix_map: the classes of the fate pass over a HEALPix source's centre rays (include/kr_trace.h has the rule)."""
    _fields_ = [(n, C.c_double) for n in ("r_isco", "r_disc", "r_esc", "theta_tol", "source_r", "source_phi", "q1", "rb1", "q2", "rb2", "q3")] + \
               [("npix", C.c_int64), ("rays_per_pixel", C.c_int32), ("self_zone", C.c_int32)]


class LineBins(C.Structure):
    """kr_line_bins: emission-line energy x time bins (include/kr_trace.h has the per-ray rules).  table_emis / table_time are host
    double arrays or None; keep the arrays alive while the struct is in use (LineBins.with_table does)."""
    _fields_ = [(n, C.c_double) for n in ("line_energy", "e_min", "de", "t0", "dt", "r_isco", "r_disc", "q1", "rb1", "q2", "rb2", "q3", "g_index",
                                          "table_r_min", "table_dr")] + \
               [("table_emis", C.POINTER(C.c_double)), ("table_time", C.POINTER(C.c_double))] + \
               [(n, C.c_int32) for n in ("ne", "nt", "log_e", "table_nr", "table_logbin", "pad")]

    def with_table(self, r_min, dr, emis, time=None, logbin=True):
        """Attach a radial emissivity (and optional source->disc time) table binned like kr_emis_bins; returns self."""
        self._table = [np.ascontiguousarray(emis, dtype=np.float64)] + ([np.ascontiguousarray(time, dtype=np.float64)] if time is not None else [])
        self.table_r_min, self.table_dr, self.table_logbin, self.table_nr = r_min, dr, int(logbin), len(self._table[0])
        self.table_emis = self._table[0].ctypes.data_as(C.POINTER(C.c_double))
        self.table_time = self._table[1].ctypes.data_as(C.POINTER(C.c_double)) if time is not None else None
        return self


class LimbLaw(C.Structure):
    """kr_limb_law: the weight of the emission angle mu in the line.  law 0: 1; 1: 1 + coeff mu; 2: log(1 + 1 / mu) (include/kr_trace.h)."""
    _fields_ = [("coeff", C.c_double), ("law", C.c_int32), ("pad", C.c_int32)]


class MuBins(C.Structure):
    """kr_mu_bins: nmu >= 1 equal bins of mu in [0, 1] (include/kr_trace.h)."""
    _fields_ = [("nmu", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(LimbLaw) == 16 and C.sizeof(MuBins) == 8

LIMB_LAWS = {"isotropic": (0, 0.0), "laor": (1, 2.06), "brightening": (2, 0.0)}


def limb_law(limb):
    """A LimbLaw from (law, coeff) or one of the names of LIMB_LAWS."""
    if isinstance(limb, LimbLaw):
        return limb
    if isinstance(limb, str):
        if limb not in LIMB_LAWS:
            raise ValueError(f"unknown limb law {limb!r}: one of {sorted(LIMB_LAWS)} or (law, coeff)")
        limb = LIMB_LAWS[limb]
    law, coeff = limb
    out = LimbLaw()
    out.law, out.coeff = int(law), float(coeff)
    return out


class DiscSurface(C.Structure):
    """kr_disc_surface: the disc surface |z| = slope rho + scale (1 - sqrt(r_in / rho)), the stop_params of STOP_THICKDISC (include/kr_trace.h)."""
    _fields_ = [("r_in", C.c_double), ("r_out", C.c_double), ("slope", C.c_double), ("scale", C.c_double)]


assert C.sizeof(DiscSurface) == 32


def disc_surface(surface):
    """A DiscSurface from (r_in, r_out, slope, scale) -- the stop_params that api.thick_disc_params sets -- or a DiscSurface."""
    if isinstance(surface, DiscSurface):
        return surface
    r_in, r_out, slope, scale = surface
    return DiscSurface(float(r_in), float(r_out), float(slope), float(scale))


class PolLaw(C.Structure):
    """kr_pol_law: the emitted polarisation degree at mu.  law 0: coeff; 1: coeff (1 - mu) / (1 + 3.582 mu) (include/kr_trace.h)."""
    _fields_ = [("coeff", C.c_double), ("law", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(PolLaw) == 16

POL_LAWS = {"full": (0, 1.0), "chandrasekhar": (1, 0.1171)}


def pol_law(pol):
    """A PolLaw from (law, coeff) or one of the names of POL_LAWS."""
    if isinstance(pol, PolLaw):
        return pol
    if isinstance(pol, str):
        if pol not in POL_LAWS:
            raise ValueError(f"unknown pol law {pol!r}: one of {sorted(POL_LAWS)} or (law, coeff)")
        pol = POL_LAWS[pol]
    law, coeff = pol
    out = PolLaw()
    out.law, out.coeff = int(law), float(coeff)
    return out


class SpectrumModel(C.Structure):
    """kr_spectrum_model: the continuum spectrum of the disc -- model 0 thermal (table_kt, f_col), model 1 a tabulated rest-frame spectrum (s, nz x s_ne
    on a log-energy grid) -- sampled at the centres of the energy bins (include/kr_trace.h has the per-ray rule).  table_kt / table_emis / s are host double
    arrays or None; keep the arrays alive while the struct is in use (spectrum_model does)."""
    _fields_ = [(n, C.c_double) for n in ("e_min", "de", "r_isco", "r_disc", "q1", "rb1", "q2", "rb2", "q3", "f_col", "table_r_min", "table_dr", "s_e_min", "s_de")] + \
               [(n, C.POINTER(C.c_double)) for n in ("table_kt", "table_emis", "s")] + \
               [(n, C.c_int32) for n in ("model", "ne", "log_e", "table_nr", "table_logbin", "s_ne", "nz", "pad")]


assert C.sizeof(SpectrumModel) == 168

SPECTRUM_MODELS = {"thermal": 0, "table": 1}


def spectrum_model(model, e_min, de, ne, log_e=False, r_isco=1.0, r_disc=1000.0, q1=3.0, rb1=4.0, q2=3.0, rb2=10.0, q3=3.0, f_col=1.0, table_r_min=0.0,
                   table_dr=0.0, table_logbin=True, table_kt=None, table_emis=None, s=None, s_e_min=0.0, s_de=0.0):
    """A SpectrumModel.  model: "thermal" / 0 (needs table_kt, binned by table_r_min, table_dr, table_logbin like kr_emis_bins) or "table" / 1 (needs s of
    shape (nz, s_ne) or (s_ne,), nodes at s_e_min s_de^k; emissivity powerlaw3 or table_emis).  The arrays are copied and kept alive by the struct."""
    m = SpectrumModel()
    m.model = SPECTRUM_MODELS.get(model, model) if isinstance(model, str) else int(model)
    m.e_min, m.de, m.ne, m.log_e = e_min, de, ne, int(log_e)
    m.r_isco, m.r_disc, m.q1, m.rb1, m.q2, m.rb2, m.q3, m.f_col = r_isco, r_disc, q1, rb1, q2, rb2, q3, f_col
    m.table_r_min, m.table_dr, m.table_logbin, m.s_e_min, m.s_de = table_r_min, table_dr, int(table_logbin), s_e_min, s_de
    m._keep = {}
    for name, a in (("table_kt", table_kt), ("table_emis", table_emis)):
        if a is not None:
            m._keep[name] = np.ascontiguousarray(a, dtype=np.float64).copy()
            setattr(m, name, m._keep[name].ctypes.data_as(C.POINTER(C.c_double)))
            m.table_nr = len(m._keep[name])
    if s is not None:
        m._keep["s"] = np.atleast_2d(np.ascontiguousarray(s, dtype=np.float64)).copy()
        m.s = m._keep["s"].ctypes.data_as(C.POINTER(C.c_double))
        m.nz, m.s_ne = m._keep["s"].shape
    return m


class ResponseModel(C.Structure):
    """kr_response_model: the energy-time response of a tabulated rest-frame spectrum -- a SpectrumModel of the table kind, the time rows (t0, dt, nt)
    and an optional source->disc time per radial bin of spec's table (include/kr_trace.h has the per-ray rule).  Keep the arrays alive while the struct
    is in use (response_model does)."""
    _fields_ = [("spec", SpectrumModel), ("t0", C.c_double), ("dt", C.c_double), ("table_time", C.POINTER(C.c_double)), ("nt", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(ResponseModel) == 200


def response_model(spec, t0, dt, nt, table_time=None):
    """A ResponseModel.  spec: a SpectrumModel made by spectrum_model("table", ...), copied in (its arrays stay alive with the result); table_time: spec.table_nr
    source->disc times binned by spec's table_r_min, table_dr, table_logbin -- with a spec that has no table_emis, table_nr is taken from its length."""
    r = ResponseModel()
    C.memmove(C.byref(r.spec), C.byref(spec), C.sizeof(SpectrumModel))
    r._keep = {"spec": getattr(spec, "_keep", None)}
    r.t0, r.dt, r.nt = t0, dt, nt
    if table_time is not None:
        r._keep["table_time"] = np.ascontiguousarray(table_time, dtype=np.float64).copy()
        r.table_time = r._keep["table_time"].ctypes.data_as(C.POINTER(C.c_double))
        if not spec.table_emis:
            r.spec.table_nr = len(r._keep["table_time"])
        elif len(r._keep["table_time"]) != spec.table_nr:
            raise ValueError("response_model: table_time must have spec.table_nr values")
    return r


class HotSpot(C.Structure):
    """kr_hotspot: a Gaussian pattern of enhanced emission that moves over the disc -- light curve, image position and spectrogram at nt observer times
    (include/kr_trace.h has the per-ray rule).  A pattern on the disc, good for sigma << r_spot; not a body with a four-velocity of its own."""
    _fields_ = [(n, C.c_double) for n in ("r_spot", "sigma", "cut", "phi0", "omega", "a_orbit", "t0", "dt", "g_index", "line_energy", "e_min", "de", "r_isco", "r_disc")] + \
               [(n, C.c_int32) for n in ("nt", "ne", "log_e", "shear")] + [("pad", C.c_int32 * 2)]


assert C.sizeof(HotSpot) == 136


def hot_spot(r_spot, sigma, cut=3.0, phi0=0.0, omega=None, shear=0, spin=0.0, t0=0.0, dt=1.0, nt=64, g_index=4.0, line_energy=6.4, e_min=1.0, de=0.1, ne=0,
             log_e=False, r_isco=1.0, r_disc=1000.0):
    """A HotSpot.  omega=None: the Keplerian rate 1 / (spin + r_spot^1.5) at the spot's centre; shear=1: every radius at its own Keplerian rate for
    `spin` (omega is then not used).  ne=0: no spectrogram."""
    h = HotSpot()
    h.r_spot, h.sigma, h.cut, h.phi0, h.a_orbit = r_spot, sigma, cut, phi0, spin
    h.omega = 1.0 / (spin + r_spot * float(np.sqrt(r_spot))) if omega is None else omega
    h.t0, h.dt, h.nt, h.g_index = t0, dt, nt, g_index
    h.line_energy, h.e_min, h.de, h.ne, h.log_e = line_energy, e_min, de, ne, int(log_e)
    h.r_isco, h.r_disc, h.shear = r_isco, r_disc, int(shear)
    return h


class CausticMap(C.Structure):
    """kr_caustic_map: what the critical-curve passes need besides the records (include/kr_trace.h has the per-pixel rules)."""
    _fields_ = [(n, C.c_double) for n in ("r_isco", "r_disc", "eps_x", "eps_y")] + [(n, C.c_int32) for n in ("nx", "ny", "bundles", "pad")]


class SourceMap(C.Structure):
    """kr_source_map: what the source-sphere / source-plane caustic pass needs besides the records (include/kr_trace.h has the per-pixel rules)."""
    _fields_ = [(n, C.c_int32) for n in ("kind", "bundles", "nx", "ny")] + [(n, C.c_double) for n in ("eps_x", "eps_y", "sin_incl", "cos_incl", "sin_phi0", "cos_phi0")]


class PathSpec(C.Structure):
    """kr_path_spec: write_step and the radial window of run_raytrace's trajectory dump (include/kr_trace.h has the write rule)."""
    _fields_ = [("write_rmin", C.c_double), ("write_rmax", C.c_double), ("write_step", C.c_int32), ("pad", C.c_int32)]


class VolumeMap(C.Structure):
    """kr_volume_map: the (r, theta, phi) grid of a volume illumination map and the observers of its energy shift (include/kr_trace.h has the rule)."""
    _fields_ = [(n, C.c_double) for n in ("r_min", "dr", "dtheta", "dphi", "V")] + \
               [(n, C.c_int32) for n in ("nr", "ntheta", "nphi", "logbin", "mode", "reverse", "projradius", "motion")]


class ObserveBins(C.Structure):
    """kr_observe_bins: the energy and time bins of an observed volume map (include/kr_trace.h has the rule)."""
    _fields_ = [(n, C.c_double) for n in ("en0", "den", "t0", "dt")] + [(n, C.c_int32) for n in ("nen", "nt", "logbin_en", "pad")]


class CrossingSpec(C.Structure):
    """kr_crossing_spec: how many equatorial crossings a recording trace stores per ray, whether the last of them ends the ray, and the emitter on the
    plane (include/kr_trace.h has the rule)."""
    _fields_ = [("V", C.c_double)] + [(n, C.c_int32) for n in ("max_crossings", "stop_when_full", "reverse", "projradius", "motion", "pad")]


class PointSourceVelSpec(C.Structure):
    """kr_pointsource_vel_spec: a point source whose emitter has any timelike four-velocity u = (u^t, u^r, u^theta, u^phi), not necessarily
    normalised (include/kr_trace.h has the tetrad, the ray rule and what is refused)."""
    _fields_ = [("pos", C.c_double * 4), ("u", C.c_double * 4)] + \
               [(n, C.c_double) for n in ("spin", "tol", "E", "dcosalpha", "dbeta", "cosalpha0", "cosalphamax", "beta0", "betamax")]


class AngdistSpec(C.Structure):
    """kr_angdist_spec: the classes and weights of kr_return_bins (cls), the bin width of the emission-angle histograms and whose (alpha, beta) labels the
    records carry -- 0: PointSource's, 1: PointSourceVel's (include/kr_trace.h)."""
    _fields_ = [("cls", ReturnBins), ("dangle", C.c_double), ("labels", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(PointSourceVelSpec) == 136 and C.sizeof(AngdistSpec) == 72


class ObserverSpec(C.Structure):
    """kr_observer_spec: the source-to-observer link -- the classes of kr_return_bins (cls), the spin of the momentum, the inclination bins of
    cos(theta_obs), the time rows, the reference sphere and the photon index (include/kr_trace.h has the rule)."""
    _fields_ = [("cls", ReturnBins)] + [(n, C.c_double) for n in ("spin", "mu0", "dmu", "t0", "dt", "dist", "gamma")] + [("nmu", C.c_int32), ("nt", C.c_int32)]


assert C.sizeof(ObserverSpec) == 120


class IllumBins(C.Structure):
    """kr_illum_bins: the (r, phi) illumination map of the disc -- the emissivity histogram's bins (rad), the azimuthal cells and the shift added to a
    record's phi before the wrap (include/kr_trace.h has the rule)."""
    _fields_ = [("rad", EmisBins), ("phi_shift", C.c_double), ("nphi", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(IllumBins) == 72


def illum_bins(rad, nphi, phi_shift=0.0):
    """An IllumBins: rad, an EmisBins, copied in; nphi cells of 2 pi / nphi from phi = -pi; phi_shift added to every record's phi before the wrap."""
    m = IllumBins()
    C.memmove(C.byref(m.rad), C.byref(rad), C.sizeof(EmisBins))
    m.phi_shift, m.nphi, m.pad = float(phi_shift), int(nphi), 0
    return m


class IllumTable(C.Structure):
    """kr_illum_table: an (r, phi) table of the emissivity and the source -> disc delay for the line and the response (include/kr_trace.h has the rule).
    emis / time are host double arrays of nr x nphi or None; keep them alive while the struct is in use (illum_table does)."""
    _fields_ = [("r_min", C.c_double), ("dr", C.c_double), ("phi_shift", C.c_double), ("emis", C.POINTER(C.c_double)), ("time", C.POINTER(C.c_double))] + \
               [(n, C.c_int32) for n in ("nr", "nphi", "logbin", "pad")]


assert C.sizeof(IllumTable) == 56


def illum_table(emis, r_min=None, dr=None, logbin=True, time=None, phi_shift=None):
    """An IllumTable from emis (and time) of shape (nr, nphi) -- or from the dict of api.illumination_table as the only argument: its planes, its radial
    grid and the phi_shift its map was made with (a cell must mean the same azimuth in the map and in the table), which the keyword replaces when
    given.  phi_shift is the orbital phase: a table made from the map of a source at phi_s = 0 with shift s serves the source at phase delta with
    phi_shift = s - delta.  The arrays are copied and kept alive by the struct."""
    if isinstance(emis, dict):
        d = emis
        emis, time, r_min, dr, logbin = d["emis"], d.get("time"), d["r_min"], d["dr"], d["logbin"]
        phi_shift = d["phi_shift"] if phi_shift is None else phi_shift
    phi_shift = 0.0 if phi_shift is None else phi_shift
    if r_min is None or dr is None:
        raise ValueError("illum_table: r_min and dr are needed with arrays")
    t = IllumTable()
    t._keep = {"emis": np.ascontiguousarray(emis, dtype=np.float64).copy()}
    if t._keep["emis"].ndim != 2:
        raise ValueError("illum_table: emis must be shaped (nr, nphi)")
    t.nr, t.nphi = t._keep["emis"].shape
    t.emis = t._keep["emis"].ctypes.data_as(C.POINTER(C.c_double))
    if time is not None:
        t._keep["time"] = np.ascontiguousarray(time, dtype=np.float64).copy()
        if t._keep["time"].shape != t._keep["emis"].shape:
            raise ValueError("illum_table: time must have the shape of emis")
        t.time = t._keep["time"].ctypes.data_as(C.POINTER(C.c_double))
    t.r_min, t.dr, t.logbin, t.phi_shift, t.pad = float(r_min), float(dr), int(bool(logbin)), float(phi_shift), 0
    return t


def line_bins(line_energy=6.4, e_min=1.0, de=0.1, ne=90, log_e=False, t0=0.0, dt=0.0, nt=1, r_isco=1.0, r_disc=1000.0, q1=3.0, rb1=4.0, q2=3.0,
              rb2=10.0, q3=3.0, g_index=3.0):
    b = LineBins()
    b.line_energy, b.e_min, b.de, b.ne, b.log_e = line_energy, e_min, de, ne, int(log_e)
    b.t0, b.dt, b.nt = t0, dt, nt
    b.r_isco, b.r_disc, b.q1, b.rb1, b.q2, b.rb2, b.q3, b.g_index = r_isco, r_disc, q1, rb1, q2, rb2, q3, g_index
    return b


def default_params(spin, horizon=None):
    """Raytracer<T> ctor defaults (reference src/raytracer/raytracer.cpp:12-22, raytracer.h:19-44)."""
    p = Params()
    p.spin = spin
    p.horizon = horizon if horizon is not None else 1.0 + np.sqrt((1.0 - spin) * (1.0 + spin))
    p.precision, p.theta_precision = 100.0, 50.0
    p.max_tstep, p.maxtstep_rlim, p.max_phistep = 1.0, 100.0, 0.1
    p.rk45_tol = 1e-8
    p.r_max, p.theta_max = 1000.0, np.pi / 2
    p.integrator, p.stop_kind, p.steplim, p.flags = EULER, STOP_THETA, -1, 0
    return p


def copy_params(p, **kw):
    q = Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(Params))
    for k, v in kw.items():
        if k == "stop_params":
            for i, x in enumerate(v):
                q.stop_params[i] = x
        else:
            setattr(q, k, v)
    return q


P = C.POINTER
_vp, _i64, _i32, _dbl, _int = C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int
PROGRESS_FN = C.CFUNCTYPE(None, C.c_int64, C.c_int64, C.c_void_p)      # kr_progress_fn

# name -> (restype, argtypes); exactly the entry points include/kr_trace.h declares
PROTOTYPES = {
    "kr_abi_version": (_int, []),
    "kr_last_error": (C.c_char_p, []),
    "kr_device_count": (_int, []),
    "kr_set_device": (_int, [_int]),
    "kr_device_info": (_int, [P(_int), P(_int), P(_i64), C.c_char_p, _int]),
    "kr_params_default": (None, [P(Params), _dbl]),
    "kr_kerr_horizon": (_dbl, [_dbl]),
    "kr_kerr_isco": (_dbl, [_dbl, _int]),
    "kr_disc_velocity": (_dbl, [_dbl, _dbl, _int]),
    "kr_plunge_flow": (_int, [_dbl, P(_dbl), P(_dbl), P(_dbl)]),
    "kr_plunge_velocity": (_int, [_dbl, _dbl, P(_dbl)]),
    "kr_pointsource_count": (_i64, [P(PointSourceSpec), P(_i32), P(_i32)]),
    "kr_imageplane_count": (_i64, [P(ImagePlaneSpec), P(_i32), P(_i32)]),
    "kr_bundles_count": (_i64, [P(ImagePlaneSpec), P(_i32), P(_i32)]),
    "kr_trace_f64": (_int, [P(Params), _vp, _i64, P(Stats)]),
    "kr_trace_f32": (_int, [P(Params), _vp, _i64, P(Stats)]),
    "kr_trace_dev_f64": (_int, [P(Params), _vp, _i64, _vp, P(Stats)]),
    "kr_trace_dev_f32": (_int, [P(Params), _vp, _i64, _vp, P(Stats)]),
    "kr_trace_async_f64": (_int, [P(Params), _vp, _i64, _vp, P(_vp)]),
    "kr_trace_async_f32": (_int, [P(Params), _vp, _i64, _vp, P(_vp)]),
    "kr_trace_batch_async_f64": (_int, [_i32, P(P(Params)), P(_vp), P(_i64), P(_vp), P(_vp)]),
    "kr_trace_wait": (_int, [_vp, P(Stats)]),
    "kr_trace_wait_many": (_int, [_i32, P(_vp), P(Stats), P(Stats)]),
    "kr_trace_release": (_int, [_vp]),
    "kr_trace_paths_count_dev_f64": (_int, [P(Params), P(PathSpec), _vp, _i64, _vp, _vp, P(_i64), _vp]),
    "kr_trace_paths_record_dev_f64": (_int, [P(Params), P(PathSpec), _vp, _i64, _vp, _vp, _i64, _vp, P(Stats)]),
    "kr_trace_paths_f64": (_int, [P(Params), P(PathSpec), _vp, _i64, _vp, _vp, P(_vp), P(_i64), P(Stats)]),
    "kr_trace_volume_dev_f64": (_int, [P(Params), P(VolumeMap), _vp, _i64, _vp, _vp, P(Stats)]),
    "kr_trace_volume_f64": (_int, [P(Params), P(VolumeMap), _vp, _i64, _vp, P(Stats)]),
    "kr_trace_observe_dev_f64": (_int, [P(Params), P(VolumeMap), P(ObserveBins), _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, P(Stats)]),
    "kr_trace_observe_f64": (_int, [P(Params), P(VolumeMap), P(ObserveBins), _vp, _vp, _vp, _vp, _i64, _vp, _vp, P(Stats)]),
    "kr_trace_crossings_dev_f64": (_int, [P(Params), P(CrossingSpec), _vp, _i64, _vp, _vp, _vp, P(Stats)]),
    "kr_trace_crossings_f64": (_int, [P(Params), P(CrossingSpec), _vp, _i64, _vp, _vp, P(Stats)]),
    "kr_reduce_crossing_image_dev_f64": (_int, [P(ImageBins), _i32, _i32, _dbl, _dbl, _vp, _vp, _vp, _i64, _vp, _vp]),
    "kr_redshift_start_f64": (_int, [_dbl, _dbl, _int, _int, _vp, _i64]),
    "kr_redshift_start_dev_f64": (_int, [_dbl, _dbl, _int, _int, _vp, _i64, _vp]),
    "kr_redshift_f64": (_int, [_dbl, _dbl, _int, _int, _int, _vp, _i64]),
    "kr_redshift_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _vp, _i64, _vp]),
    "kr_redshift_dest_f64": (_int, [_dbl, _int, _vp, _i64]),
    "kr_redshift_dest_dev_f64": (_int, [_dbl, _int, _vp, _i64, _vp]),
    "kr_range_phi_f64": (_int, [_dbl, _dbl, _vp, _i64]),
    "kr_range_phi_dev_f64": (_int, [_dbl, _dbl, _vp, _i64, _vp]),
    "kr_calculate_momentum_f64": (_int, [_dbl, _vp, _i64]),
    "kr_calculate_momentum_dev_f64": (_int, [_dbl, _vp, _i64, _vp]),
    "kr_redshift_start_f32": (_int, [_dbl, _dbl, _int, _int, _vp, _i64]),
    "kr_redshift_start_dev_f32": (_int, [_dbl, _dbl, _int, _int, _vp, _i64, _vp]),
    "kr_redshift_f32": (_int, [_dbl, _dbl, _int, _int, _int, _vp, _i64]),
    "kr_redshift_dev_f32": (_int, [_dbl, _dbl, _int, _int, _int, _vp, _i64, _vp]),
    "kr_redshift_dest_f32": (_int, [_dbl, _int, _vp, _i64]),
    "kr_redshift_dest_dev_f32": (_int, [_dbl, _int, _vp, _i64, _vp]),
    "kr_range_phi_f32": (_int, [_dbl, _dbl, _vp, _i64]),
    "kr_range_phi_dev_f32": (_int, [_dbl, _dbl, _vp, _i64, _vp]),
    "kr_calculate_momentum_f32": (_int, [_dbl, _vp, _i64]),
    "kr_calculate_momentum_dev_f32": (_int, [_dbl, _vp, _i64, _vp]),
    "kr_pointsource_init_f64": (_int, [P(PointSourceSpec), _vp, _i64]),
    "kr_pointsource_init_dev_f64": (_int, [P(PointSourceSpec), _vp, _i64, _vp]),
    "kr_imageplane_init_f64": (_int, [P(ImagePlaneSpec), _vp, _i64]),
    "kr_imageplane_init_dev_f64": (_int, [P(ImagePlaneSpec), _vp, _i64, _vp]),
    "kr_pointsource_init_strided_dev_f64": (_int, [P(PointSourceSpec), _i64, _i64, _vp, _i64, _vp]),
    "kr_imageplane_init_strided_dev_f64": (_int, [P(ImagePlaneSpec), _i64, _i64, _vp, _i64, _vp]),
    "kr_reduce_emissivity_f64": (_int, [P(EmisBins), _vp, _i64, _vp, _vp, _vp, _vp, _vp, P(_i64)]),
    "kr_reduce_emissivity_dev_f64": (_int, [P(EmisBins), _vp, _i64, _vp, _vp]),
    "kr_pointsource_init_emit_dev_f64": (_int, [P(PointSourceSpec), _i64, _i64, _dbl, _int, _int, _vp, _i64, _vp]),
    "kr_imageplane_init_emit_dev_f64": (_int, [P(ImagePlaneSpec), _i64, _i64, _dbl, _int, _int, _vp, _i64, _vp]),
    "kr_imageplane_init_emit_runs_dev_f64": (_int, [P(ImagePlaneSpec), _i64, _i64, _i64, _dbl, _int, _int, _vp, _i64, _vp]),
    "kr_post_image_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(ImageBins), _vp, _i64, _vp, _vp]),
    "kr_trace_poll": (_int, [_vp, P(_i64), P(_i32)]),
    "kr_trace_progress_f64": (_int, [P(Params), _vp, _i64, P(Stats), _i64, PROGRESS_FN, _vp]),
    "kr_trace_progress_f32": (_int, [P(Params), _vp, _i64, P(Stats), _i64, PROGRESS_FN, _vp]),
    "kr_pointsource_tables": (_int, [P(PointSourceSpec), _vp, _vp, _vp]),
    "kr_post_emissivity_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(EmisBins), _vp, _i64, _vp, _vp]),
    "kr_reduce_image_f64": (_int, [P(ImageBins), _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, P(_i64)]),
    "kr_reduce_image_dev_f64": (_int, [P(ImageBins), _vp, _i64, _vp, _vp]),
    "kr_reduce_emissivity_surface_dev_f64": (_int, [P(EmisBins), _vp, _i64, _vp, _vp]),
    "kr_post_emissivity_surface_dev_f64": (_int, [_dbl, _int, _dbl, _dbl, P(EmisBins), _vp, _i64, _vp, _vp]),
    "kr_reduce_image_surface_dev_f64": (_int, [P(ImageBins), _vp, _i64, _vp, _vp]),
    "kr_post_image_surface_dev_f64": (_int, [_dbl, _int, _dbl, _dbl, P(ImageBins), _vp, _i64, _vp, _vp]),
    "kr_reduce_return_f64": (_int, [P(ReturnBins), _vp, _i64, P(_dbl * 4)]),
    "kr_reduce_return_dev_f64": (_int, [P(ReturnBins), _vp, _i64, _vp, _vp]),
    "kr_post_return_dev_f64": (_int, [_dbl, _dbl, P(ReturnBins), _vp, _i64, _vp, _vp]),
    "kr_post_return_batch_dev_f64": (_int, [_i32, _dbl, _dbl, P(ReturnBins), P(_vp), P(_i64), P(_vp), _vp]),
    "kr_pointsource_init_emit_batch_dev_f64": (_int, [_i32, P(PointSourceSpec), P(_dbl), _int, _int, P(_vp), P(_i64), _vp]),
    "kr_reduce_return_map_f64": (_int, [P(ReturnMap), _vp, _i64, _vp]),
    "kr_reduce_return_map_dev_f64": (_int, [P(ReturnMap), _vp, _i64, _vp, _vp]),
    "kr_post_return_map_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(ReturnMap), _vp, _i64, _vp, _vp]),
    "kr_post_return_map_batch_dev_f64": (_int, [_i32, _dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(ReturnMap), P(_vp), P(_i64), P(_vp), _vp]),
    "kr_healpix_count": (_i64, [P(HealpixSource), P(_i64)]),
    "kr_healpix_vectors_dev_f64": (_int, [_i32, _i32, _i64, _i64, _i64, _vp, _vp]),
    "kr_healpix_init_dev_f64": (_int, [P(HealpixSource), _i64, _i64, _vp, _i64, _vp]),
    "kr_healpix_init_emit_dev_f64": (_int, [P(HealpixSource), _i64, _i64, _int, _vp, _i64, _vp]),
    "kr_healpix_init_f64": (_int, [P(HealpixSource), _vp, _i64]),
    "kr_post_healpix_map_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(HealpixMap), _vp, _i64, _i64, _i64, _vp, _vp]),
    "kr_reduce_healpix_map_dev_f64": (_int, [P(HealpixMap), _vp, _i64, _i64, _i64, _vp, _vp]),
    "kr_reduce_healpix_map_f64": (_int, [P(HealpixMap), _vp, _i64, _vp]),
    "kr_pointsource_vel_count": (_i64, [P(PointSourceVelSpec), P(_i32), P(_i32)]),
    "kr_pointsource_vel_tetrad": (_int, [P(PointSourceVelSpec), _vp]),
    "kr_pointsource_vel_init_dev_f64": (_int, [P(PointSourceVelSpec), _vp, _i64, _vp]),
    "kr_pointsource_vel_init_emit_dev_f64": (_int, [P(PointSourceVelSpec), _vp, _i64, _vp]),
    "kr_pointsource_vel_init_f64": (_int, [P(PointSourceVelSpec), _vp, _i64]),
    "kr_angdist_nangle": (_int, [P(AngdistSpec)]),
    "kr_post_angdist_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(AngdistSpec), _vp, _i64, _vp, _vp]),
    "kr_reduce_angdist_dev_f64": (_int, [P(AngdistSpec), _vp, _i64, _vp, _vp]),
    "kr_reduce_angdist_f64": (_int, [P(AngdistSpec), _vp, _i64, _vp]),
    "kr_post_observer_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(ObserverSpec), _vp, _i64, _vp, _vp]),
    "kr_reduce_observer_dev_f64": (_int, [P(ObserverSpec), _vp, _i64, _vp, _vp]),
    "kr_reduce_observer_f64": (_int, [P(ObserverSpec), _vp, _i64, _vp]),
    "kr_post_illum_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(IllumBins), _vp, _i64, _vp, _vp]),
    "kr_reduce_illum_dev_f64": (_int, [P(IllumBins), _vp, _i64, _vp, _vp]),
    "kr_reduce_illum_f64": (_int, [P(IllumBins), _vp, _i64, _vp]),
    "kr_post_line_illum_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(LineBins), P(LimbLaw), P(IllumTable), _vp, _i64, _vp, _vp]),
    "kr_reduce_line_illum_dev_f64": (_int, [P(LineBins), P(IllumTable), _vp, _i64, _vp, _vp]),
    "kr_reduce_line_illum_f64": (_int, [P(LineBins), P(IllumTable), _vp, _i64, _vp]),
    "kr_post_response_illum_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(ResponseModel), P(LimbLaw), P(IllumTable), _vp, _i64, _vp, _vp]),
    "kr_reduce_response_illum_dev_f64": (_int, [P(ResponseModel), P(IllumTable), _vp, _i64, _vp, _vp]),
    "kr_reduce_response_illum_f64": (_int, [P(ResponseModel), P(IllumTable), _vp, _i64, _vp]),
    "kr_reduce_line_f64": (_int, [P(LineBins), _vp, _i64, _vp]),
    "kr_reduce_line_dev_f64": (_int, [P(LineBins), _vp, _i64, _vp, _vp]),
    "kr_post_line_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(LineBins), _vp, _i64, _vp, _vp]),
    "kr_line_from_image_dev_f64": (_int, [P(LineBins), P(ImageBins), _vp, _vp, _vp]),
    "kr_angles_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _vp, _i64, _vp, _vp]),
    "kr_angles_f64": (_int, [_dbl, _dbl, _int, _int, _int, _vp, _i64, _vp]),
    "kr_post_line_limb_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(LineBins), P(LimbLaw), _vp, _i64, _vp, _vp]),
    "kr_post_emissivity_mu_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(EmisBins), P(MuBins), _vp, _i64, _vp, _vp, _vp]),
    "kr_polarisation_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _vp, _i64, _vp, _vp]),
    "kr_polarisation_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _vp, _i64, _vp]),
    "kr_post_image_stokes_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, _dbl, P(ImageBins), P(LimbLaw), P(PolLaw), _vp, _i64, _vp, _vp]),
    "kr_post_line_stokes_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, _dbl, P(LineBins), P(LimbLaw), P(PolLaw), _vp, _i64, _vp, _vp]),
    "kr_post_spectrum_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(SpectrumModel), P(LimbLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_spectrum_dev_f64": (_int, [P(SpectrumModel), _vp, _i64, _vp, _vp]),
    "kr_reduce_spectrum_f64": (_int, [P(SpectrumModel), _vp, _i64, _vp]),
    "kr_post_spectrum_stokes_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, _dbl, P(SpectrumModel), P(LimbLaw), P(PolLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_spectrum_stokes_dev_f64": (_int, [_dbl, _dbl, _int, _int, _dbl, P(SpectrumModel), P(LimbLaw), P(PolLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_spectrum_stokes_f64": (_int, [_dbl, _dbl, _int, _int, _dbl, P(SpectrumModel), P(LimbLaw), P(PolLaw), _vp, _i64, _vp]),
    "kr_post_response_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(ResponseModel), P(LimbLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_response_dev_f64": (_int, [P(ResponseModel), _vp, _i64, _vp, _vp]),
    "kr_reduce_response_f64": (_int, [P(ResponseModel), _vp, _i64, _vp]),
    "kr_angles_surface_dev_f64": (_int, [P(DiscSurface), _dbl, _int, _vp, _i64, _vp, _vp]),
    "kr_angles_surface_f64": (_int, [P(DiscSurface), _dbl, _int, _vp, _i64, _vp]),
    "kr_post_line_surface_dev_f64": (_int, [P(DiscSurface), _dbl, _int, _dbl, _dbl, P(LineBins), P(LimbLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_line_surface_dev_f64": (_int, [P(DiscSurface), P(LineBins), _vp, _i64, _vp, _vp]),
    "kr_post_spectrum_surface_dev_f64": (_int, [P(DiscSurface), _dbl, _int, _dbl, _dbl, P(SpectrumModel), P(LimbLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_spectrum_surface_dev_f64": (_int, [P(DiscSurface), P(SpectrumModel), _vp, _i64, _vp, _vp]),
    "kr_reduce_spectrum_surface_f64": (_int, [P(DiscSurface), P(SpectrumModel), _vp, _i64, _vp]),
    "kr_post_response_surface_dev_f64": (_int, [P(DiscSurface), _dbl, _int, _dbl, _dbl, P(ResponseModel), P(LimbLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_response_surface_dev_f64": (_int, [P(DiscSurface), P(ResponseModel), _vp, _i64, _vp, _vp]),
    "kr_reduce_response_surface_f64": (_int, [P(DiscSurface), P(ResponseModel), _vp, _i64, _vp]),
    "kr_post_hotspot_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, P(HotSpot), P(LimbLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_hotspot_dev_f64": (_int, [P(HotSpot), _vp, _i64, _vp, _vp]),
    "kr_reduce_hotspot_f64": (_int, [P(HotSpot), _vp, _i64, _vp]),
    "kr_post_hotspot_stokes_dev_f64": (_int, [_dbl, _dbl, _int, _int, _int, _dbl, _dbl, _dbl, P(HotSpot), P(LimbLaw), P(PolLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_hotspot_stokes_dev_f64": (_int, [_dbl, _dbl, _int, _int, _dbl, P(HotSpot), P(LimbLaw), P(PolLaw), _vp, _i64, _vp, _vp]),
    "kr_reduce_hotspot_stokes_f64": (_int, [_dbl, _dbl, _int, _int, _dbl, P(HotSpot), P(LimbLaw), P(PolLaw), _vp, _i64, _vp]),
    "kr_bundles_init_emit_dev_f64": (_int, [P(ImagePlaneSpec), _dbl, _dbl, _int, _int, _vp, _i64, _vp]),
    "kr_post_caustic_disc_dev_f64": (_int, [_dbl, _int, P(CausticMap), _vp, _i64, _vp, _vp]),
    "kr_caustic_suppress_dev_f64": (_int, [P(CausticMap), _vp, _vp]),
    "kr_post_caustic_source_dev_f64": (_int, [P(SourceMap), _vp, _i64, _vp, _vp]),
    "kr_debug_arith_f64": (_int, [_int, _vp, _vp, _vp, _i64]),
    "kr_host_attach": (_int, [_vp, _i64, _i32]),
    "kr_host_detach": (_int, [_vp]),
    "kr_malloc": (_int, [P(_vp), _i64]),
    "kr_free": (_int, [_vp]),
    "kr_host_alloc": (_int, [P(_vp), _i64]),
    "kr_host_free": (_int, [_vp]),
    "kr_memcpy_h2d": (_int, [_vp, _vp, _i64]),
    "kr_memcpy_d2h": (_int, [_vp, _vp, _i64]),
    "kr_memset": (_int, [_vp, _int, _i64]),
    "kr_synchronize": (_int, [_vp]),
    "kr_stream_create": (_int, [P(_vp)]),
    "kr_stream_destroy": (_int, [_vp]),
    "kr_configure_process": (_int, []),
    "kr_shutdown": (_int, []),
}

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libkrtrace.so")


class KrError(RuntimeError):
    pass


def load(path=None):
    """dlopen libkrtrace.so and attach prototypes.  Raises if the library or any declared symbol is missing."""
    path = path or os.environ.get("KRTRACE_LIB") or LIB_PATH      # KRTRACE_LIB: an experiment build (scripts/ab_kernels.py)
    if not os.path.exists(path):
        raise KrError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise KrError(f"{path} does not export {name} (declared in include/kr_trace.h)") from e
        fn.restype, fn.argtypes = res, args
    if lib.kr_abi_version() != ABI_VERSION:
        raise KrError(f"ABI mismatch: library {lib.kr_abi_version()} vs binding {ABI_VERSION}")
    return lib


def check(lib, rc, what):
    if rc != KR_OK:
        msg = lib.kr_last_error()
        raise KrError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")
