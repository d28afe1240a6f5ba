"""Host-side mirror of py21cmfast's driver layer for the boxes this backend computes: the evolution
loop of ``run_coeval`` (reference: src/py21cmfast/drivers/coeval.py:560-890) as ``run_coeval`` /
``Inputs`` below, and the bookkeeping that sits between the C entry points of the
spin-temperature path for the Lagrangian source models
(reference: src/py21cmfast/drivers/single_field.py:382-470 ``interp_halo_boxes`` and :473-636
``compute_xray_source_field``), and the rectilinear lightcone of ``run_lightcone``
(reference: src/py21cmfast/lightconers.py, drivers/lightcone.py) with its slabs and dv/dr correction on
the device, and its angular lightcone (AngularLightconer), interpolated on the device.  A py21cmfast installation keeps using its own drivers on top of
the library; this module is for callers without it (tests, tools, stand-alone runs).

The reference does this bookkeeping in Python with astropy: the shells of the X-ray / Lyman-alpha
light cone are placed in comoving distance, every shell takes the halo grids (``halo_sfr``,
``halo_xray``) linearly interpolated between the two snapshots that bracket its mean redshift,
and ``UpdateXraySourceBox`` filters them into ``XraySourceBox.filtered_sfr / filtered_xray``.
astropy is not a dependency here: the comoving distance of its ``FlatLambdaCDM`` (photons plus
three neutrino species, one of 0.06 eV, as in its Planck18 realisation) is restated with numpy.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import structs as S
from ._lib import check, load

L_FACTOR = (4 * math.pi / 3.0) ** (-1 / 3)  # single_field.py:516
C_KMS = 299792.458
MPC_CM = 3.085677581491367e24  # astropy's Mpc
G_CGS = 6.6743e-8              # CODATA 2018, as astropy.constants
M_P = 1.67262192369e-24
SIGMA_SB = 5.670374419e-5
C_CMS = 2.99792458e10
K_B_EV = 8.617333262e-5


class FlatCosmology:
    """astropy.cosmology.FlatLambdaCDM(H0, Om0, Ob0, Tcmb0 = 2.7255 K, Neff = 3.046,
    m_nu = [0, 0, 0.06] eV) -- what ``CosmoParams.cosmo`` is for the Planck18 base
    (reference: wrapper/inputs.py:603-611).  Only E(z) and the comoving distance are needed."""

    def __init__(self, hlittle, OMm, Tcmb0=2.7255, Neff=3.046, m_nu=(0.0, 0.0, 0.06)):
        self.h, self.Om0 = float(hlittle), float(OMm)
        self.H0_cgs = self.h * 100.0 * 1e5 / MPC_CM  # 1/s
        self.rho_crit0 = 3 * self.H0_cgs**2 / (8 * math.pi * G_CGS)  # g / cm^3
        a_rad = 4 * SIGMA_SB / C_CMS
        self.Ogamma0 = a_rad * Tcmb0**4 / (self.rho_crit0 * C_CMS**2)
        m = np.array(m_nu, float)
        self.n_massless = int(np.sum(m == 0))
        self.nu_y = m[m > 0] / (K_B_EV * 0.7137658555036082 * Tcmb0)
        self.neff_per_nu = Neff / 3.0
        self.Onu0 = self.Ogamma0 * self._nu_rel(0.0)
        self.Ode0 = 1.0 - self.Om0 - self.Ogamma0 - self.Onu0

    def _nu_rel(self, z):
        """Komatsu et al. 2011 eq. 26 as astropy evaluates it (nu_relative_density)."""
        p, invp, k = 1.83, 0.54644808743, 0.3173
        z = np.asarray(z, float)
        y = self.nu_y[None, :] / (1.0 + z[..., None]) if z.ndim else self.nu_y / (1.0 + z)
        rel = np.sum((1.0 + (k * y) ** p) ** invp, axis=-1) + self.n_massless
        return 0.22710731766 * self.neff_per_nu * rel

    def efunc(self, z):
        z = np.asarray(z, float)
        zp1 = 1.0 + z
        return np.sqrt(zp1**3 * (self.Ogamma0 * (1 + self._nu_rel(z)) * zp1 + self.Om0) + self.Ode0)

    def comoving_distance(self, z):
        """Mpc; composite Gauss-Legendre in ln(1 + z), converged to ~1e-10."""
        x, w = np.polynomial.legendre.leggauss(12)
        out = []
        for zz in np.atleast_1d(np.asarray(z, float)):
            edges = np.linspace(0.0, math.log1p(zz), 17)
            tot = 0.0
            for a, b in zip(edges[:-1], edges[1:]):
                u = 0.5 * (a + b) + 0.5 * (b - a) * x
                tot += 0.5 * (b - a) * float(np.sum(w * np.exp(u) / self.efunc(np.expm1(u))))
            out.append(C_KMS / (100.0 * self.h) * tot)
        return np.array(out) if np.ndim(z) else out[0]

    def z_at_comoving_distance(self, d):
        lo, hi = 0.0, 2000.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if self.comoving_distance(mid) < d:
                lo = mid
            else:
                hi = mid
            if hi - lo < 1e-12 * max(1.0, hi):
                break
        return 0.5 * (lo + hi)


def xray_shells(redshift, hii_dim, box_len, n_step, r_max_ts, cosmo: FlatCosmology):
    """Outer radii [Mpc] and mean redshifts of the shells (single_field.py:515-546): edges in
    comoving distance from `redshift`, converted with a 100-point log grid in z, mean = outer
    edge minus half the shell's redshift width."""
    R_min = (1.5 if hii_dim == 1 else box_len / hii_dim) * L_FACTOR
    steps = np.arange(0, n_step)
    R_range = R_min * (r_max_ts / R_min) ** (steps / n_step)
    cmd_edges = cosmo.comoving_distance(redshift) + R_range
    zmin = cosmo.z_at_comoving_distance(cmd_edges.min())
    zmax = cosmo.z_at_comoving_distance(cmd_edges.max())
    zgrid = np.logspace(np.log10(zmin), np.log10(zmax), 100)
    dgrid = cosmo.comoving_distance(zgrid)
    zpp_edges = np.interp(cmd_edges, dgrid, zgrid)
    zpp_avg = zpp_edges - np.diff(np.insert(zpp_edges, 0, redshift)) / 2
    return R_range, zpp_avg


def interp_halo_boxes(z_halos, boxes, fields, redshift):
    """Linear interpolation of the halo grids between the two snapshots bracketing `redshift`
    (single_field.py:382-470).  z_halos ascending; boxes: dicts of arrays.  Returns a dict."""
    z_halos = list(z_halos)
    if not np.all(np.diff(z_halos) > 0):
        raise ValueError("halo_boxes must be in ascending order of redshift")
    if redshift > z_halos[-1] or redshift < z_halos[0]:
        raise ValueError(f"Invalid z_target {redshift} for redshift array {z_halos}")
    idx_prog = int(np.searchsorted(z_halos, redshift, side="left"))
    if idx_prog == 0 or idx_prog == len(z_halos):
        raise ValueError(f"redshift {redshift} beyond limits {z_halos[0], z_halos[-1]}")
    idx_desc = idx_prog - 1
    t = (redshift - z_halos[idx_desc]) / (z_halos[idx_prog] - z_halos[idx_desc])
    out = {}
    for f in fields:
        if np.ndim(boxes[idx_desc][f]) == 0:  # box-level scalars (log10_Mcrit_MCG_ave)
            out[f] = (1 - t) * boxes[idx_desc][f] + t * boxes[idx_prog][f]
            continue
        a, b = boxes[idx_desc][f], boxes[idx_prog][f]
        if hasattr(a, "is_cuda"):  # torch tensors: the history stays in HBM
            out[f] = ((1 - t) * a + t * b).contiguous()
            continue
        interp = np.zeros_like(a)
        interp[...] = (1 - t) * a + t * b
        out[f] = interp
    return out


def lya_diffusion_scale(redshift, x_HI, hlittle, OMm, OMb, Y_He, cosmo: FlatCosmology):
    """R_star [Mpc] of the multiple-scattering window, eq. 24 of arXiv:2601.14360 as coded at
    single_field.py:549-572."""
    A_alpha, nu_Lya = 6.25e8, 2.46606727e15
    n_H_z0 = (1.0 - Y_He) * cosmo.rho_crit0 * OMb / M_P
    R = 3.0 * C_CMS**4 * A_alpha**2 * n_H_z0 * x_HI * (1.0 + redshift)
    R /= 32.0 * math.pi**3 * nu_Lya**4 * cosmo.H0_cgs**2 * OMm
    return R / MPC_CM


def compute_xray_source_field(z_halos, hboxes, redshift, *, simulation_options, cosmo_params,
                              astro_params, astro_options, previous_xHI_mean=None, lib=None):
    """XraySourceBox for `redshift` from the halo-grid history (compute_xray_source_field,
    single_field.py:473-636).  `z_halos` / `hboxes`: redshifts (descending, as the evolution
    produces them, the current one last) and dicts with ``halo_sfr`` and ``halo_xray`` grids (with
    USE_MINI_HALOS also ``halo_sfr_mini`` and the scalar ``log10_Mcrit_MCG_ave``).
    The process-global parameters must have been broadcast to the library.  Returns a dict with
    ``filtered_sfr``, ``filtered_xray`` [N_STEP_TS, ...] and ``mean_sfr`` [N_STEP_TS] (mini-halos:
    ``filtered_sfr_mini``, ``mean_log10_Mcrit_LW`` and, under LYA_MULTIPLE_SCATTERING, the
    straight-line copies ``filtered_sfr_lw`` / ``filtered_sfr_mini_lw``)."""
    lib = lib or load(require_gpu=True)
    so, cp, ap, ao = simulation_options, cosmo_params, astro_params, astro_options
    mini = bool(ao.USE_MINI_HALOS)
    n_step = ap.N_STEP_TS
    shape = tuple(hboxes[0]["halo_sfr"].shape)
    on_device = hasattr(hboxes[0]["halo_sfr"], "is_cuda")  # torch history: zero-copy entry points
    if on_device:
        import torch

        dev = hboxes[0]["halo_sfr"].device

        def grid_stack():
            return torch.zeros((n_step,) + shape, dtype=torch.float32, device=dev)

        def fptr(a):
            return C.cast(a.data_ptr(), S.c_float_p)

        def all_zero(a):
            return not bool(torch.any(a != 0))
    else:
        def grid_stack():
            return np.zeros((n_step,) + shape, np.float32)

        def fptr(a):
            return a.ctypes.data_as(S.c_float_p)

        def all_zero(a):
            return bool(np.all(a == 0))
    cosmo = FlatCosmology(cp.hlittle, cp.OMm)
    R_range, zpp_avg = xray_shells(redshift, so.HII_DIM, so.BOX_LEN, n_step, ap.R_MAX_TS, cosmo)
    z_max = min(max(z_halos), so.Z_HEAT_MAX)
    if ao.LYA_MULTIPLE_SCATTERING:
        x_HI = 1.0 if previous_xHI_mean is None else float(previous_xHI_mean)
        R_star = lya_diffusion_scale(redshift, x_HI, cp.hlittle, cp.OMm, cp.OMb, cp.Y_He, cosmo)
    else:
        R_star = 0.0
    box = {"filtered_sfr": grid_stack(), "filtered_xray": grid_stack(),
           "mean_sfr": np.zeros(n_step), "mean_sfr_mini": np.zeros(n_step),
           "mean_log10_Mcrit_LW": np.zeros(n_step)}
    extra = {}
    if mini:
        names = ["filtered_sfr_mini"] + (["filtered_sfr_lw", "filtered_sfr_mini_lw"]
                                         if ao.LYA_MULTIPLE_SCATTERING else [])
        for k in names:
            box[k] = grid_stack()
            extra[k] = fptr(box[k])
    src = S.XraySourceBoxStruct(
        filtered_sfr=fptr(box["filtered_sfr"]), filtered_xray=fptr(box["filtered_xray"]), **extra,
        mean_sfr=box["mean_sfr"].ctypes.data_as(C.POINTER(C.c_double)),
        mean_sfr_mini=box["mean_sfr_mini"].ctypes.data_as(C.POINTER(C.c_double)),
        mean_log10_Mcrit_LW=box["mean_log10_Mcrit_LW"].ctypes.data_as(C.POINTER(C.c_double)))
    order = np.argsort(z_halos)
    z_sorted = [z_halos[i] for i in order]
    b_sorted = [hboxes[i] for i in order]
    for i in range(n_step):
        R_inner = float(R_range[i - 1]) if i > 0 else 0.0
        R_outer = float(R_range[i])
        if zpp_avg[i] >= z_max:  # above Z_HEAT_MAX or the first snapshot: nothing shines yet
            if mini:  # "minimum" (single_field.py:591; upstream's M_TURN is the log10 there)
                box["mean_log10_Mcrit_LW"][i] = math.log10(ap.M_TURN)
            continue
        fields = ("halo_sfr", "halo_xray") + (("halo_sfr_mini", "log10_Mcrit_MCG_ave") if mini else ())
        hb = interp_halo_boxes(z_sorted, b_sorted, fields, float(zpp_avg[i]))
        if all_zero(hb["halo_sfr"]) and (not mini or all_zero(hb["halo_sfr_mini"])):
            if mini:
                box["mean_log10_Mcrit_LW"][i] = hb["log10_Mcrit_MCG_ave"]
            continue
        hbs = S.HaloBoxStruct(halo_sfr=fptr(hb["halo_sfr"]), halo_xray=fptr(hb["halo_xray"]))
        if mini:
            hbs.halo_sfr_mini = fptr(hb["halo_sfr_mini"])
            hbs.log10_Mcrit_MCG_ave = float(hb["log10_Mcrit_MCG_ave"])
        check(lib.UpdateXraySourceBox(C.byref(hbs), R_inner, R_outer, i, R_star, C.byref(src)),
              "UpdateXraySourceBox")
    box["zpp_avg"], box["R_range"], box["R_star"] = zpp_avg, R_range, R_star
    return box


# =============================================================================================
# The evolution loop (reference: src/py21cmfast/drivers/coeval.py:749-890 `_redshift_loop_generator`
# with `run_coeval`'s set-up :560-745, and drivers/_global_initialization.py for the C state).
# =============================================================================================
TS_FIELDS = ("spin_temperature", "kinetic_temp_neutral", "xray_ionised_fraction")
ION_FIELDS = ("neutral_fraction", "z_reion", "kinetic_temperature", "unnormalised_nion",
              "ionisation_rate_G12", "mean_free_path", "cumulative_recombinations")


def ionisation_radii(so, ap, lagrangian: bool, ionise_entire_sphere: bool = False) -> int:
    """Number of filter radii of the excursion set (setup_radii, IonisationBox.c:964-1006): the
    length of IonizedBox.unnormalised_nion[_mini] with USE_MINI_HALOS."""
    L_FACTOR = 0.620350491
    pixel = float(so.BOX_LEN) / float(so.HII_DIM)
    r_max = min(float(ap.R_BUBBLE_MAX), L_FACTOR * float(so.BOX_LEN))
    # setup_radii, IonisationBox.c:968-972: the unit cell factor only without IONISE_ENTIRE_SPHERE
    cell_factor = 1.0 if (lagrangian and pixel < 1 and not ionise_entire_sphere) else L_FACTOR
    r_min = max(float(ap.R_BUBBLE_MIN), cell_factor * pixel)
    n_radii = int(math.log(r_max / r_min) / math.log(float(ap.DELTA_R_HII_FACTOR)) + 1)
    for i in range(n_radii):
        if r_min * float(ap.DELTA_R_HII_FACTOR) ** i > r_max - 1e-7:
            return i + 1
    return n_radii


def get_logspaced_redshifts(min_redshift, z_step_factor, max_redshift):
    """The node redshifts of an evolution, descending (wrapper/inputs.py:1774-1789)."""
    z = 10 ** np.arange(np.log10(1 + min_redshift), np.log10((1 + max_redshift) * z_step_factor),
                        np.log10(z_step_factor)) - 1
    return tuple(float(v) for v in z[::-1])


class Inputs:
    """The six parameter structs of a run (InputParameters, wrapper/inputs.py) with the defaults
    of ``structs.default_*``; keyword arguments are routed to the struct that has the field."""

    def __init__(self, random_seed=1, cosmo_tables=None, **kw):
        groups = (("simulation_options", S.SimulationOptions, S.default_simulation_options),
                  ("matter_options", S.MatterOptions, S.default_matter_options),
                  ("cosmo_params", S.CosmoParams, S.default_cosmo_params),
                  ("astro_params", S.AstroParams, S.default_astro_params),
                  ("astro_options", S.AstroOptions, S.default_astro_options))
        for name, cls, make in groups:
            names = {f[0] for f in cls._fields_}
            setattr(self, name, make(**{k: kw.pop(k) for k in list(kw) if k in names}))
        if kw:
            raise TypeError(f"unknown parameters: {sorted(kw)}")
        self.cosmo_tables = cosmo_tables or S.default_cosmo_tables()
        self.random_seed = int(random_seed)

    @property
    def evolution_required(self):
        """Whether a box depends on the previous snapshot (wrapper/inputs.py:1805-1815)."""
        return bool(self.astro_options.USE_TS_FLUCT or self.astro_options.RECOMB_MODEL != 0)

    def node_redshifts(self, out_redshifts):
        so = self.simulation_options
        if not self.evolution_required:
            return tuple(sorted((float(z) for z in out_redshifts), reverse=True))
        return get_logspaced_redshifts(min(out_redshifts), so.ZPRIME_STEP_FACTOR, so.Z_HEAT_MAX)



def required_redshifts(inputs: "Inputs", out_redshifts):
    """_get_required_redshifts_coeval (coeval.py:971-992): the node redshifts above the lowest
    requested one plus the requested redshifts themselves, descending and unique (float32 values,
    as the C entry points take them).  A requested redshift that is not a node is an extra
    snapshot computed at exactly that z; it does NOT become the next snapshot's "previous" box
    and its halo grids do not enter the history (coeval.py:880-884).  Returns (all_redshifts,
    set of those that are nodes)."""
    outs = [float(np.float32(z)) for z in out_redshifts]
    nodes = [float(np.float32(z)) for z in inputs.node_redshifts(outs)]
    if not inputs.evolution_required:
        allz = sorted(set(outs), reverse=True)
        return allz, set(allz)
    nodes = [z for z in nodes if z > min(outs)]
    return sorted(set(nodes) | set(outs), reverse=True), set(nodes)


def _initialise(lib, inputs: Inputs, data_path):
    """What GlobalInitializationManager does before the first Compute* call."""
    i = inputs
    lib.Broadcast_struct_global_all(*(C.byref(x) for x in (
        i.simulation_options, i.matter_options, i.cosmo_params, i.astro_params, i.astro_options,
        i.cosmo_tables)))
    if data_path is not None:
        i._data_path = str(data_path).encode()  # kept alive: C holds the pointer
        S.ConfigSettings.in_dll(lib, "config_settings").external_table_path = i._data_path
    lib.init_ps()
    if i.astro_options.USE_TS_FLUCT:
        lib.init_heat.restype = C.c_int
        if lib.init_heat() != 0:
            check(1, "init_heat")
    elif data_path is not None:
        lib.c21_recfast_load.restype = C.c_int
        check(lib.c21_recfast_load(), "recfast")
    if i.astro_options.RECOMB_MODEL != 0:
        lib.init_MHR.restype = None
        lib.init_MHR()


class PerturbedHalos:
    """What ``perturb_halo_catalog`` returns: ``n_halos`` and one array per field of the reference's
    PerturbedHaloCatalog (``halo_coords`` [n_halos, 3] in Mpc, the others [n_halos]); a field that the
    options switch off is None.  ``struct`` is the C struct the arrays belong to."""

    def __init__(self, struct):
        self.struct, self.n_halos = struct, int(struct.n_halos)
        for name in S.PERTURBED_HALO_FIELDS:
            a = struct.arrays.get(name)
            setattr(self, name, None if a is None else a[:self.n_halos])

    def fields(self):
        return {k: getattr(self, k) for k in S.PERTURBED_HALO_FIELDS if getattr(self, k) is not None}


def _box_struct(cls, box):
    """A TsBox / IonizedBox struct from None, a struct or a dict of arrays by field name."""
    from . import grid_api as api

    if box is None or isinstance(box, cls):
        return box
    names = {f[0] for f in cls._fields_}
    st = cls(**{k: api._fptr(v) for k, v in box.items() if k in names and hasattr(v, "shape")})
    st._keep = box
    return st


def _perturb_halos(lib, inputs, redshift, icss, catalog, prev_ts, prev_ion, device):
    """ComputePerturbedHaloCatalog with the globals already broadcast."""
    lib.ComputePerturbedHaloCatalog.restype = C.c_int
    lib.ComputePerturbedHaloCatalog.argtypes = [C.c_float] + [C.c_void_p] * 5
    out = S.perturbed_halo_catalog(int(catalog.n_halos), inputs, device=device)
    check(lib.ComputePerturbedHaloCatalog(float(redshift), C.byref(icss),
                                          C.byref(prev_ts) if prev_ts is not None else None,
                                          C.byref(prev_ion) if prev_ion is not None else None,
                                          C.byref(catalog), C.byref(out)), "ComputePerturbedHaloCatalog")
    return PerturbedHalos(out)


def perturb_halo_catalog(inputs: Inputs, redshift, ics, catalog, prev_ts=None, prev_ion=None, *,
                         data_path=None, device=None, lib=None):
    """The halos of ``catalog`` (``structs.halo_catalog``; numpy or device arrays) at their Eulerian
    positions at ``redshift`` with their stellar masses, star-formation rates, ionising and X-ray
    emissivities (reference: ``perturb_halo_catalog``, drivers/single_field.py; C:
    PerturbedHaloCatalog.c:25-149, HaloBox.c:781-880), for SOURCE_MODEL = DEXM-ESF / CHMF-SAMPLER.
    Row i belongs to halo i; halos of zero mass get coordinates and zeros elsewhere.

    ``ics``: the initial conditions, as ``run_coeval`` returns them under ``"initial_conditions"`` (a
    dict of arrays) or an InitialConditionsStruct.  ``prev_ts`` / ``prev_ion``: the previous snapshot's
    TsBox / IonizedBox (structs, or dicts of arrays by field name), read with USE_MINI_HALOS below
    Z_HEAT_MAX only.  ``device``: where the output arrays live (None: numpy).  Returns a
    ``PerturbedHalos``."""
    from . import grid_api as api

    lib = lib or load(require_gpu=True)
    i = inputs
    lib.Broadcast_struct_global_all(*(C.byref(x) for x in (
        i.simulation_options, i.matter_options, i.cosmo_params, i.astro_params, i.astro_options,
        i.cosmo_tables)))
    if data_path is not None:
        i._data_path = str(data_path).encode()  # kept alive: C holds the pointer
        S.ConfigSettings.in_dll(lib, "config_settings").external_table_path = i._data_path
    lib.init_ps()
    icss = ics if isinstance(ics, S.InitialConditionsStruct) else api.ics_struct(ics)
    return _perturb_halos(lib, inputs, redshift, icss, catalog, _box_struct(S.TsBoxStruct, prev_ts),
                          _box_struct(S.IonizedBoxStruct, prev_ion), device)


HALO_CATALOG_MEM_FACTOR = 1.2  # the reference's default (py21cmfast config)
HALO_CATALOG_MIN_ROWS = 1000000  # get_halo_catalog_buffer_size (wrapper/cfuncs.py:57-79)


def _halo_catalog(lib, redshift, icss, desc, seed, mem_factor, device):
    """ComputeHaloCatalog with the globals already broadcast: the buffer holds (expected_nhalo + 1) times
    ``mem_factor`` rows, at least HALO_CATALOG_MIN_ROWS."""
    lib.expected_nhalo.restype = C.c_double
    lib.expected_nhalo.argtypes = [C.c_double]
    lib.ComputeHaloCatalog.restype = C.c_int
    lib.ComputeHaloCatalog.argtypes = [C.c_float, C.c_float, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_void_p]
    factor = HALO_CATALOG_MEM_FACTOR if mem_factor is None else float(mem_factor)
    S.ConfigSettings.in_dll(lib, "config_settings").HALO_CATALOG_MEM_FACTOR = factor  # named by the overflow error
    expected = lib.expected_nhalo(float(redshift))
    if not np.isfinite(expected):
        raise ValueError(f"expected_nhalo({redshift}) is not finite: the inputs describe no box")
    rows = max(int((expected + 1.0) * factor), HALO_CATALOG_MIN_ROWS)
    out = S.empty_halo_catalog(rows, device=device)
    z_desc = -1.0 if desc is None else float(desc.redshift)
    check(lib.ComputeHaloCatalog(z_desc, float(redshift), C.byref(icss), int(seed),
                                 C.byref(desc) if desc is not None else None, C.byref(out)), "ComputeHaloCatalog")
    out.redshift = float(redshift)
    return out


def _evolve_halos(lib, inputs, all_redshifts, is_node, icss, mem_factor, device):
    """evolve_halos with the globals already broadcast"""
    cats, desc = {}, None
    for z in sorted(all_redshifts):  # lowest first: every node is the descendant of the next one up
        cats[z] = _halo_catalog(lib, z, icss, desc, inputs.random_seed, mem_factor, device)
        if z in is_node:
            desc = cats[z]
    return cats


def determine_halo_catalog(inputs: Inputs, redshift, ics, descendant_halos=None, mem_factor=None, lib=None,
                           device=None, data_path=None):
    """The halo catalogue of one snapshot (reference: ``determine_halo_catalog``, drivers/single_field.py; C:
    ComputeHaloCatalog).  SOURCE_MODEL = DEXM-ESF: the DexM finder on ``ics["hires_density"]``.
    CHMF-SAMPLER: with ``descendant_halos`` (a catalogue this function returned for a LOWER redshift) the
    progenitors of its halos; without, the DexM halos of the snapshot followed by the halos sampled in
    every cell of ``ics["lowres_density"]``.

    ``ics``: the initial conditions (a dict of arrays as ``run_coeval`` returns them under
    ``"initial_conditions"``, or an InitialConditionsStruct).  The buffer holds ``(expected_nhalo(z) + 1) *
    mem_factor`` rows (default: the reference's HALO_CATALOG_MEM_FACTOR of 1.2), at least a million.
    Returns a ``structs.HaloCatalogStruct`` with ``n_halos`` set, its arrays under ``.arrays`` (numpy, or
    torch tensors on ``device``) and its ``.redshift``."""
    from . import grid_api as api

    lib = lib or load(require_gpu=True)
    if inputs.matter_options.SOURCE_MODEL not in (3, 4):
        raise ValueError("SOURCE_MODEL has no halo catalogues")
    _initialise(lib, inputs, data_path)
    icss = ics if isinstance(ics, S.InitialConditionsStruct) else api.ics_struct(ics)
    return _halo_catalog(lib, float(np.float32(redshift)), icss, descendant_halos, inputs.random_seed, mem_factor,
                         device)


def evolve_halos(inputs: Inputs, all_redshifts, ics, *, nodes=None, mem_factor=None, lib=None, device=None,
                 data_path=None):
    """The halo catalogues of a run (reference: ``evolve_halos``, drivers/coeval.py:435-517): the redshifts
    are walked lowest first; the lowest gets the DexM halos and the sampled cells, every other one the
    progenitors of the last NODE below it (``nodes``: the redshifts that are nodes; default: all of them).
    Returns ``{z: HaloCatalogStruct}`` keyed by the float32 redshifts."""
    from . import grid_api as api

    lib = lib or load(require_gpu=True)
    if inputs.matter_options.SOURCE_MODEL not in (3, 4):
        return {}
    _initialise(lib, inputs, data_path)
    icss = ics if isinstance(ics, S.InitialConditionsStruct) else api.ics_struct(ics)
    zs = [float(np.float32(z)) for z in all_redshifts]
    is_node = set(zs) if nodes is None else {float(np.float32(z)) for z in nodes}
    return _evolve_halos(lib, inputs, zs, is_node, icss, mem_factor, device)


def run_coeval(inputs: Inputs, out_redshifts, *, data_path=None, device=None, lib=None,
               keep=("density", "velocity_z", "neutral_fraction", "z_reion", "brightness_temp") + TS_FIELDS,
               progress=None, halo_catalogs=None, inspect=None, keep_perturbed_halos=False):
    """Evolve boxes through the library's entry points, mirroring ``run_coeval``: initial
    conditions once, then from the highest node redshift down: PerturbedField -> [HaloBox ->
    XraySourceBox ->] [TsBox ->] IonizedBox -> BrightnessTemp, every snapshot receiving the
    previous one's boxes.  Supported source models: CONST-ION-EFF, E-INTEGRAL, L-INTEGRAL and,
    with catalogues from the caller, DEXM-ESF / CHMF-SAMPLER: ``halo_catalogs(z)`` returns the
    catalogue of node redshift z as ``structs.HaloCatalogStruct`` (``structs.halo_catalog``; numpy or
    device arrays), or ``halo_catalogs="sample"`` finds and samples them from the initial conditions first
    (``evolve_halos``).

    ``device``: a torch device string ("cuda") keeps every array in HBM (zero-copy entry points);
    None uses numpy arrays that the library stages.  ``data_path``: directory of the reference's
    data tables (py21cmfast's ``_data``).  Returns ``{redshift: {field: array}}`` for the requested
    redshifts (fields in ``keep``, and ``velocity_x`` / ``velocity_y`` with KEEP_3D_VELOCITIES; plus the
    scalars ``mean_f_coll`` and ``Q_HI``), keyed by the
    requested redshift as float32 -- a requested redshift between two nodes is computed AT that
    redshift from the last node above it, like upstream -- and, under the key ``"history"``, the
    global signal (z, mean dT_b, mean x_HI, mean T_s) of every snapshot computed.
    ``inspect(z, ctx)``: test hook called after every snapshot with the structs its
    ComputeIonizedBox call was given (``ctx["new_ion"]()`` allocates another output box).
    ``keep_perturbed_halos``: with a catalogue source model, every requested redshift also gets
    ``"perturbed_halos"``: its catalogue moved and converted (``perturb_halo_catalog``)."""
    lib = lib or load(require_gpu=True)
    out_redshifts = [float(np.float32(z)) for z in out_redshifts]
    all_redshifts, is_node = required_redshifts(inputs, out_redshifts)
    wanted = set(out_redshifts)
    result, history = {}, []
    mini = bool(inputs.astro_options.USE_MINI_HALOS)
    snaps = _snapshots(inputs, all_redshifts, is_node, inputs.evolution_required, data_path=data_path,
                       device=device, lib=lib, progress=progress, halo_catalogs=halo_catalogs,
                       inspect=inspect, history=history, perturbed_halos=keep_perturbed_halos)
    if inputs.matter_options.KEEP_3D_VELOCITIES:  # the two extra components come back with velocity_z
        keep = tuple(keep) + tuple(k for k in ("velocity_x", "velocity_y") if k not in keep)
    ics = None
    for z, boxes, ion, ts, ics in snaps:
        if z in wanted:
            snap = {k: boxes[k] for k in keep if k in boxes}
            snap["mean_f_coll"], snap["Q_HI"] = ion.mean_f_coll, ts.Q_HI
            if mini:
                snap["mean_f_coll_MINI"] = ion.mean_f_coll_MINI
                snap["log10_Mturnover_ave"] = ion.log10_Mturnover_ave
                snap["log10_Mturnover_MINI_ave"] = ion.log10_Mturnover_MINI_ave
            if "perturbed_halos" in boxes:
                snap["perturbed_halos"] = boxes["perturbed_halos"]
            result[z] = snap
    result["history"] = history
    result["initial_conditions"] = ics
    return result


class Coeval:
    """A thin view of one snapshot of ``run_coeval`` (Coeval, drivers/coeval.py:44-377): ``inputs``, the
    ``redshift`` and the snapshot's ``fields`` (name -> array, numpy or torch), each field reachable as an
    attribute.  Its three methods are the reference's velocity corrections (:242-377), run on the device
    where the arrays live.

    As upstream, ``axis`` only selects WHICH velocity component enters (``velocity_x`` / ``_y`` / ``_z``):
    the gradient and the shift always run along the LAST axis of the box, whatever ``axis`` says."""

    def __init__(self, inputs: Inputs, redshift, fields: dict):
        self.inputs, self.redshift, self.fields = inputs, float(redshift), dict(fields)

    @classmethod
    def from_result(cls, result: dict, redshift, inputs: Inputs) -> "Coeval":
        """The snapshot of ``redshift`` out of what ``run_coeval(inputs, ...)`` returned."""
        return cls(inputs, redshift, result[float(np.float32(redshift))])

    def __getattr__(self, name):
        fields = self.__dict__.get("fields", {})
        if name in fields:
            return fields[name]
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def _los_velocity(self, axis):
        if not hasattr(self, "velocity_" + str(axis)):
            if axis not in ["x", "y", "z"]:
                raise ValueError("`axis` can only be `x`, `y` or `z`.")
            raise ValueError("You asked for axis = '" + axis + "', but the coeval doesn't have velocity_" + axis
                             + "! Set matter_options.KEEP_3D_VELOCITIES=True next time you call run_coeval if "
                             "you wish to set axis=`" + axis + "'.")
        return getattr(self, "velocity_" + axis)

    def _tau_21(self):
        if not self.inputs.astro_options.USE_TS_FLUCT:
            return None
        if "tau_21" not in self.fields:
            raise ValueError('USE_TS_FLUCT needs the tau_21 box of the snapshot: pass keep=(..., "tau_21") to '
                             "run_coeval")
        return self.fields["tau_21"]

    def include_dvdr_in_tau21(self, axis: str = "z", periodic: bool = True):
        """The brightness temperature with the velocity-gradient correction (coeval.py:242-278)."""
        from . import rsds

        vel = self._los_velocity(axis)
        return rsds.include_dvdr_in_tau21(self.brightness_temp, vel, self.redshift, self.inputs,
                                          periodic=periodic, tau_21=self._tau_21())

    def apply_rsds(self, field: str = "brightness_temp", axis: str = "z", periodic: bool = True,
                   n_rsd_subcells: int = 4):
        """``field`` of the box with redshift-space distortions (coeval.py:280-326)."""
        from . import rsds

        vel = self._los_velocity(axis)
        return rsds.apply_rsds(getattr(self, field), vel, self.redshift, self.inputs, periodic=periodic,
                               n_rsd_subcells=n_rsd_subcells)

    def apply_velocity_corrections(self, axis: str = "z", periodic: bool = True, n_rsd_subcells: int = 4):
        """The brightness temperature with the velocity-gradient correction, then redshift-space
        distortions (coeval.py:328-377)."""
        from . import rsds

        vel = self._los_velocity(axis)
        tb = rsds.include_dvdr_in_tau21(self.brightness_temp, vel, self.redshift, self.inputs,
                                        periodic=periodic, tau_21=self._tau_21())
        return rsds.apply_rsds(tb, vel, self.redshift, self.inputs, periodic=periodic,
                               n_rsd_subcells=n_rsd_subcells)


def _snapshots(inputs: Inputs, all_redshifts, is_node, chain, *, data_path, device, lib, progress,
               halo_catalogs, inspect, history, perturbed_halos=False):
    """The per-snapshot body shared by ``run_coeval`` and ``run_lightcone``: yields
    ``(z, boxes, ion, ts, ics)`` for every redshift of ``all_redshifts`` (descending), ``boxes`` the
    snapshot's arrays by name, ``ion`` / ``ts`` its IonizedBox / TsBox structs.  A node (``z in
    is_node``) becomes the next snapshot's "previous" one when ``chain`` is true (run_coeval: only
    for evolution runs, coeval.py:878-884; a lightcone: always).  Appends the global signal
    (z, mean dT_b, mean x_HI, mean T_s) of every snapshot to ``history``.  ``perturbed_halos``: with a
    catalogue source model ``boxes["perturbed_halos"]`` holds the snapshot's PerturbedHalos."""
    from . import grid_api as api

    so, mo, ao, ap = (inputs.simulation_options, inputs.matter_options, inputs.astro_options,
                      inputs.astro_params)
    if mo.SOURCE_MODEL in (3, 4) and halo_catalogs is None:
        raise NotImplementedError("SOURCE_MODEL = DEXM-ESF / CHMF-SAMPLER needs halo_catalogs: a function of "
                                  "the redshift, or \"sample\" to find and sample them (evolve_halos)")
    mini = bool(ao.USE_MINI_HALOS)
    if mini and not (mo.SOURCE_MODEL in (1, 2, 3, 4) and ao.USE_TS_FLUCT):
        raise NotImplementedError("USE_MINI_HALOS runs with SOURCE_MODEL = E-INTEGRAL or L-INTEGRAL "
                                  "and USE_TS_FLUCT (the Lyman-Werner background comes from the TsBox)")
    _initialise(lib, inputs, data_path)
    n, nz = so.HII_DIM, int(so.NON_CUBIC_FACTOR * so.HII_DIM)
    shape = (n, n, nz)
    lagrangian, ts_on, recomb = mo.SOURCE_MODEL >= 2, bool(ao.USE_TS_FLUCT), ao.RECOMB_MODEL
    n_radii = ionisation_radii(so, ap, lagrangian, bool(ao.IONISE_ENTIRE_SPHERE))
    if device is not None:
        import torch

        def new(fill=0.0, shp=shape):
            return torch.full(shp, fill, dtype=torch.float32, device=device)

        def host(a):
            return a.cpu().numpy()
    else:
        def new(fill=0.0, shp=shape):
            return np.full(shp, fill, np.float32)

        def host(a):
            return a
    fp = api._fptr

    spec = S.IcsSpec(dim=so.DIM, dim_z=int(so.NON_CUBIC_FACTOR * so.DIM), hii_dim=n, hii_dim_z=nz,
                     perturb_algorithm=mo.PERTURB_ALGORITHM, perturb_on_high_res=int(mo.PERTURB_ON_HIGH_RES))
    ics = api.new_ics_arrays(spec, device=device)
    if mo.V_CB_MODEL == 1:
        ics["lowres_vcb"] = new()
    icss = api.ics_struct(ics)
    check(lib.ComputeInitialConditions(inputs.random_seed, C.byref(icss)), "ComputeInitialConditions")
    if isinstance(halo_catalogs, str):
        if halo_catalogs != "sample":
            raise ValueError('halo_catalogs is a function of the redshift, or "sample"')
        halo_catalogs = _evolve_halos(lib, inputs, all_redshifts, is_node, icss, None, device).__getitem__

    lib.ComputeTsBox.restype = C.c_int
    lib.ComputeTsBox.argtypes = [C.c_float, C.c_float, C.c_float, C.c_short] + [C.c_void_p] * 5
    lib.ComputeHaloBox.restype = C.c_int
    lib.ComputeHaloBox.argtypes = [C.c_double] + [C.c_void_p] * 5
    lib.ComputeBrightnessTemp.restype = C.c_int
    lib.ComputeBrightnessTemp.argtypes = [C.c_float] + [C.c_void_p] * 4

    def new_ion():
        rshape = shape if recomb != 1 else (1, 1, 1)
        arr = {k: new(1.0 if k == "neutral_fraction" else 0.0,
                      rshape if k == "cumulative_recombinations" else shape) for k in ION_FIELDS}
        if mini and not lagrangian:  # one f_coll grid per radius and population (outputs.py:1538-1543)
            arr["unnormalised_nion"] = new(0.0, (n_radii,) + shape)
            arr["unnormalised_nion_mini"] = new(0.0, (n_radii,) + shape)
        if mo.MINIMIZE_MEMORY:
            arr.pop("kinetic_temperature"), arr.pop("mean_free_path")
        return arr, S.IonizedBoxStruct(**{k: fp(v) for k, v in arr.items()})

    def new_ts():
        arr = {k: new() for k in TS_FIELDS + (("J_21_LW",) if mini else ())}
        return arr, S.TsBoxStruct(**{k: fp(v) for k, v in arr.items()})

    prev_ion_arr, prev_ion = new_ion()
    prev_ts_arr, prev_ts = new_ts()
    prev_pf_arr = None
    prev_z, prev_xHI = 0.0, None
    prev_means = (0.0, 0.0)
    z_halos, hboxes = [], []
    pf_fields = ("density", "velocity_z") + (("velocity_x", "velocity_y") if mo.KEEP_3D_VELOCITIES else ())
    for z in all_redshifts:
        pf_arr = {k: new() for k in pf_fields}
        pf = S.PerturbedFieldStruct(**{k: fp(v) for k, v in pf_arr.items()})
        check(lib.ComputePerturbedField(z, C.byref(icss), C.byref(pf)), "ComputePerturbedField")
        hb_arr, hb, moved = {}, S.HaloBoxStruct(), {}
        if lagrangian:
            names = (["n_ion", "halo_sfr"] + (["halo_xray"] if ts_on else [])
                     + (["whalo_sfr"] if recomb else []) + (["halo_sfr_mini"] if mini else []))
            hb_arr = {k: new() for k in names}
            hb = S.HaloBoxStruct(**{k: fp(v) for k, v in hb_arr.items()})
            # (mini-halos: turnover masses from the previous snapshot's J_21_LW, Gamma_12, z_reion)
            cat = halo_catalogs(z) if mo.SOURCE_MODEL in (3, 4) else None
            check(lib.ComputeHaloBox(z, C.byref(icss), C.byref(cat) if cat is not None else None,
                                     C.byref(prev_ts) if mini else None,
                                     C.byref(prev_ion) if mini else None, C.byref(hb)),
                  "ComputeHaloBox")
            if perturbed_halos and cat is not None:
                moved["perturbed_halos"] = _perturb_halos(lib, inputs, z, icss, cat, prev_ts if mini else None,
                                                          prev_ion if mini else None, device)
        ts_arr, ts = ({}, S.TsBoxStruct())
        if ts_on:
            srcs = None
            if lagrangian:  # the X-ray light cone reads the halo-grid HISTORY (host arrays)
                # (device runs keep the history in HBM: interpolation and filtering never leave it)
                hist = {k: hb_arr[k] for k in ("halo_sfr", "halo_xray")
                        + (("halo_sfr_mini",) if mini else ())}
                if mini:
                    hist["log10_Mcrit_MCG_ave"] = hb.log10_Mcrit_MCG_ave
                xsrc = compute_xray_source_field(
                    z_halos + [z], hboxes + [hist], z, simulation_options=so,
                    cosmo_params=inputs.cosmo_params, astro_params=ap, astro_options=ao,
                    previous_xHI_mean=prev_xHI, lib=lib)
                srcs = S.XraySourceBoxStruct(filtered_sfr=fp(xsrc["filtered_sfr"]),
                                             filtered_xray=fp(xsrc["filtered_xray"]))
                if mini:
                    for k in ("filtered_sfr_mini", "filtered_sfr_lw", "filtered_sfr_mini_lw"):
                        if k in xsrc:
                            setattr(srcs, k, fp(xsrc[k]))
                    srcs.mean_log10_Mcrit_LW = xsrc["mean_log10_Mcrit_LW"].ctypes.data_as(
                        C.POINTER(C.c_double))
                if z in is_node:  # hbox_arr grows on the nodes only (coeval.py:880-884)
                    z_halos.append(z)
                    hboxes.append(hist)
            ts_arr, ts = new_ts()
            check(lib.ComputeTsBox(z, prev_z, z, 0, C.byref(pf), C.byref(srcs) if srcs else None,
                                   C.byref(prev_ts), C.byref(icss), C.byref(ts)), "ComputeTsBox")
        ion_arr, ion = new_ion()
        if prev_pf_arr is None and mini:
            # the first snapshot's "previous" field is a dummy that ComputeIonizedBox overwrites
            # with -1.5 (IonisationBox.c:394-398): it must not alias the current density
            prev_pf_arr = {k: new() for k in pf_fields}
        if mini:  # the trapezoidal means live in the structs (set_mean_fcoll, :476-501)
            prev_ion.mean_f_coll, prev_ion.mean_f_coll_MINI = prev_means
        prev_pf = S.PerturbedFieldStruct(**{k: fp(v) for k, v in (prev_pf_arr or pf_arr).items()})
        check(lib.ComputeIonizedBox(z, prev_z, C.byref(pf), C.byref(prev_pf), C.byref(prev_ion),
                                    C.byref(ts), C.byref(hb), C.byref(icss), C.byref(ion)),
              "ComputeIonizedBox")
        bt_arr = {"brightness_temp": new(), "tau_21": new()}
        bt = S.BrightnessTempStruct(**{k: fp(v) for k, v in bt_arr.items()})
        check(lib.ComputeBrightnessTemp(z, C.byref(ts), C.byref(ion), C.byref(pf), C.byref(bt)),
              "ComputeBrightnessTemp")
        mean = lambda a: float(a.double().mean()) if device is not None else float(a.mean(dtype=np.float64))  # noqa: E731
        prev_xHI = mean(ion_arr["neutral_fraction"])
        history.append((z, mean(bt_arr["brightness_temp"]), prev_xHI,
                        mean(ts_arr["spin_temperature"]) if ts_on else float("nan")))
        if progress:
            progress(history[-1])
        if inspect:  # test hook: the structs of this snapshot's ComputeIonizedBox call, before they age
            inspect(z, dict(prev_z=prev_z, pf=pf, prev_pf=prev_pf, prev_ion=prev_ion, ts=ts, hb=hb,
                            icss=icss, ion=ion, ion_arr=ion_arr, ts_arr=ts_arr, pf_arr=pf_arr,
                            new_ion=new_ion))
        yield z, {**pf_arr, **hb_arr, **ts_arr, **ion_arr, **bt_arr, **moved}, ion, ts, ics
        if z in is_node:
            prev_means = (ion.mean_f_coll, ion.mean_f_coll_MINI)
        if chain and z in is_node:  # only nodes are the next one's "previous"
            prev_ts_arr, prev_ts, prev_ion_arr, prev_ion, prev_pf_arr, prev_z = (
                ts_arr, ts, ion_arr, ion, pf_arr, z)


# =============================================================================================
# Lightcones (reference: src/py21cmfast/lightconers.py:36-319,483-529,541-701 and
# drivers/lightcone.py:172-181,249-277,544-575).  The slabs, the angular sampling, the spline prefilter
# and the dv/dr correction are HIP kernels (csrc/hip/lightcone_kernels.hip,
# angular_lightcone_kernels.hip); the geometry below is the host's.
# =============================================================================================
class _Lightconer:
    """What both lightconers share (Lightconer, lightconers.py:36-160): the slice distances
    ``lc_distances`` [Mpc], their redshifts, the quantities and their interpolation kinds, and which
    slices lie between two nodes with their redshift-interpolation weights."""

    def _init_common(self, lc_distances, quantities, cosmo, interp_kinds):
        self.lc_distances = np.asarray(lc_distances, float)
        if self.lc_distances.ndim != 1 or len(self.lc_distances) == 0:
            raise ValueError("lc_distances must be a non-empty 1-D array")
        if np.any(self.lc_distances < 0):
            raise ValueError("lc_distances must be non-negative")
        if cosmo is None:
            cp = S.default_cosmo_params()
            cosmo = FlatCosmology(cp.hlittle, cp.OMm)
        self.cosmo = cosmo
        self.quantities = tuple(quantities)
        self.interp_kinds = {"z_reion": "mean_max"} if interp_kinds is None else dict(interp_kinds)
        for k, v in self.interp_kinds.items():
            if v not in ("mean", "mean_max"):
                raise ValueError(f"interp_kinds[{k!r}] must be 'mean' or 'mean_max'")
        self._lc_redshifts = None

    @classmethod
    def between_redshifts(cls, min_redshift, max_redshift, resolution, quantities=("brightness_temp",),
                          cosmo=None, **kw):
        """Regular comoving-distance slices ``resolution`` [Mpc] apart from ``min_redshift`` to
        past ``max_redshift`` (lightconers.py:116-131)."""
        if cosmo is None:
            cp = S.default_cosmo_params()
            cosmo = FlatCosmology(cp.hlittle, cp.OMm)
        d0 = cosmo.comoving_distance(float(min_redshift))
        d1 = cosmo.comoving_distance(float(max_redshift))
        res = float(resolution)
        return cls(lc_distances=np.arange(d0, d1 + res, res), quantities=quantities, cosmo=cosmo, **kw)

    @property
    def lc_redshifts(self) -> np.ndarray:
        """Redshift of every slice: z at the two ends, np.interp on a 100-point log grid in between
        (lightconers.py:89-101, drivers/lightcone.py:172-181)."""
        if self._lc_redshifts is None:
            d = self.lc_distances
            zmin = self.cosmo.z_at_comoving_distance(d.min())
            zmax = self.cosmo.z_at_comoving_distance(d.max())
            zgrid = np.logspace(np.log10(zmin), np.log10(zmax), 100)
            self._lc_redshifts = np.interp(d, self.cosmo.comoving_distance(zgrid), zgrid)
        return self._lc_redshifts

    def _extended_distances(self, n_low: int, n_high: int):
        """lc_distances with ``n_low`` / ``n_high`` more slices at the low- / high-redshift end, spaced
        as its own end slices; None when both are 0."""
        n_low, n_high = int(n_low), int(n_high)
        if n_low < 0 or n_high < 0:
            raise ValueError("the buffer slice counts must be >= 0")
        d = self.lc_distances
        if (n_low or n_high) and len(d) < 2:
            raise ValueError("a lightcone of one slice has no spacing to extend it by")
        if not (n_low or n_high):
            return None
        lo = d[0] - (d[1] - d[0]) * np.arange(n_low, 0, -1)
        hi = d[-1] + (d[-1] - d[-2]) * np.arange(1, n_high + 1)
        return np.concatenate([lo, d, hi])

    def pair_slices(self, z_lo, z_hi, cell_size):
        """The slices between the nodes at ``z_lo`` < ``z_hi`` and their redshift-interpolation weights
        (make_lightcone_slices :189-207, redshift_interpolation :307-309): returns (idx, lcd, w_lo, w_hi,
        w_norm) -- the slice indices [i0, i1), their distances, |dc_hi - d|, |dc_lo - d| and |dc_lo - dc_hi|
        in pixels of ``cell_size`` [Mpc] -- or None when no slice lies between the two."""
        pix = self.lc_distances / float(cell_size)
        dc_lo = self.cosmo.comoving_distance(float(z_lo)) / float(cell_size)
        dc_hi = self.cosmo.comoving_distance(float(z_hi)) / float(cell_size)
        dcmin, dcmax = min(dc_lo, dc_hi), max(dc_lo, dc_hi)
        # tolerance at the low-redshift end: the last slice may sit exactly on the lowest node
        idx = np.nonzero((pix >= dcmin * (1 - 1e-6)) & (pix < dcmax))[0]
        if len(idx) == 0:
            return None
        if np.any(np.diff(idx) != 1):
            raise ValueError("lc_distances must be increasing")
        lcd = pix[idx]
        return idx, lcd, np.abs(dc_hi - lcd), np.abs(dc_lo - lcd), abs(dc_lo - dc_hi)


class RectilinearLightconer(_Lightconer):
    """Slices at comoving distances ``lc_distances`` [Mpc] along the last axis of the node boxes
    (RectilinearLightconer, lightconers.py:483-529).  ``index_offset`` (default: the number of
    slices) places the back of the lightcone on the back of the node box; ``interp_kinds`` maps a
    quantity to "mean" (default) or "mean_max" (``z_reion``).  ``cosmo``: a FlatCosmology, by
    default that of the default CosmoParams."""

    def __init__(self, lc_distances, quantities=("brightness_temp",), cosmo=None, index_offset=None,
                 interp_kinds=None):
        self._init_common(lc_distances, quantities, cosmo, interp_kinds)
        self.index_offset = len(self.lc_distances) if index_offset is None else int(index_offset)

    def get_shape(self, simulation_options) -> tuple:
        return (int(simulation_options.HII_DIM), int(simulation_options.HII_DIM), len(self.lc_distances))

    def extended(self, n_low: int, n_high: int) -> "RectilinearLightconer":
        """This lightconer with ``n_low`` / ``n_high`` more slices at the low- / high-redshift end,
        spaced as its own end slices; ``index_offset`` is kept, as the reference's attrs.evolve keeps
        it (lightconers.py:395-400), so the node-box planes of the slices follow the new back."""
        d = self._extended_distances(n_low, n_high)
        if d is None:
            return self
        return RectilinearLightconer(d, quantities=self.quantities, cosmo=self.cosmo,
                                     index_offset=self.index_offset, interp_kinds=self.interp_kinds)

    def lightcone_dimensions(self, simulation_options) -> tuple:
        """(x, y, line of sight) extent in Mpc (LightCone.lightcone_dimensions)."""
        so = simulation_options
        cell = float(so.BOX_LEN) / float(so.HII_DIM)
        return (float(so.BOX_LEN), float(so.BOX_LEN), len(self.lc_distances) * cell)

    def slab_tables(self, z_lo, z_hi, cell_size, d_para):
        """The slices between the nodes at ``z_lo`` < ``z_hi`` and how to fill them
        (make_lightcone_slices :189-207, coeval_subselect :505-515, redshift_interpolation :307-309):
        returns (i0, plane, w_lo, w_hi, w_norm), or None when no slice lies between the two.
        Distances are in pixels of ``cell_size`` [Mpc]; ``plane`` indexes the node boxes' last axis
        (``d_para`` planes, wrapped)."""
        pair = self.pair_slices(z_lo, z_hi, cell_size)
        if pair is None:
            return None
        idx, lcd, w_lo, w_hi, w_norm = pair
        pix = self.lc_distances / float(cell_size)
        lcidx = np.array([int(v) for v in (pix.max() - lcd + 1)], np.int64)
        plane = np.mod(-lcidx + self.index_offset, int(d_para)).astype(np.int32)
        return int(idx[0]), plane, w_lo, w_hi, w_norm


# the rotation of AngularLightconer.like_rectilinear: scipy's Rotation.from_euler("Y", -pi/2), which maps
# the direction (b, l) = (0, 0) to +z
LIKE_RECTILINEAR_ROTATION = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])


def _rotation_matrix(rotation):
    """A 3 x 3 rotation matrix from None, a matrix or anything with ``as_matrix()`` (scipy's Rotation)."""
    if rotation is None:
        return None
    R = np.array(rotation.as_matrix() if hasattr(rotation, "as_matrix") else rotation, dtype=np.float64)
    if R.shape != (3, 3) or not np.all(np.isfinite(R)) or not np.allclose(R @ R.T, np.eye(3), atol=1e-9) \
            or not np.isclose(np.linalg.det(R), 1.0, atol=1e-9):
        raise ValueError("rotation must be a 3x3 rotation matrix (or have as_matrix())")
    return R


class AngularLightconer(_Lightconer):
    """Slices at comoving distances ``lc_distances`` [Mpc] sampled in the directions (``latitude``,
    ``longitude``) [rad] (AngularLightconer, lightconers.py:541-701).  The direction
    u = (cos b cos l, cos b sin l, sin b) is rotated by ``rotation`` (a 3 x 3 matrix, anything with
    ``as_matrix()`` such as scipy's Rotation, or None); pixel p of the slice at d sits at
    x = d n_p / cell + ``origin`` [cells] of the periodic node boxes and takes their B-spline
    interpolation of ``interpolation_order`` (0, 1, 3 or 5) there.  ``los_velocity`` is the
    projection of the 3-D velocity on n_p (KEEP_3D_VELOCITIES).  The lightcones have shape
    (n_pix, n_slices)."""

    def __init__(self, latitude, longitude, lc_distances, quantities=("brightness_temp",), cosmo=None,
                 interpolation_order=1, origin=(0.0, 0.0, 0.0), rotation=None, interp_kinds=None):
        self._init_common(lc_distances, quantities, cosmo, interp_kinds)
        self.latitude = np.asarray(latitude, float)
        self.longitude = np.asarray(longitude, float)
        # the reference's validators (lightconers.py:566-573), in its order
        if self.longitude.ndim != 1:
            raise ValueError("longitude must be 1-dimensional")
        if np.any(self.longitude < 0) or np.any(self.longitude > 2 * np.pi):
            raise ValueError("longitude must be in the range [0, 2pi]")
        if self.longitude.shape != self.latitude.shape:
            raise ValueError("longitude and latitude must have the same shape")
        if not np.all(np.isfinite(self.latitude)):
            raise ValueError("latitude must be finite")
        order = int(interpolation_order)
        if order not in (0, 1, 3, 5):
            raise ValueError(f"'interpolation_order' must be in [0, 1, 3, 5] (got {interpolation_order!r})")
        self.interpolation_order = order
        self.origin = np.asarray(origin, float)
        if self.origin.shape != (3,) or not np.all(np.isfinite(self.origin)):
            raise ValueError("origin must be three finite coordinates [pixels]")
        self.rotation = _rotation_matrix(rotation)
        self._nhat = None

    @classmethod
    def like_rectilinear(cls, simulation_options, match_at_z, max_redshift, cosmo=None, **kw):
        """An angular lightconer with the pixel size of a rectilinear one (lightconers.py:579-635): an
        HII_DIM x HII_DIM grid of angles spanning BOX_LEN at ``match_at_z`` (latitude decreasing along the
        rows), the rotation that maps (0, 0) to +z and the origin that puts the slice at ``match_at_z`` on
        plane 0 of the node boxes; slices one cell apart from ``match_at_z`` to ``max_redshift``."""
        so = simulation_options
        if cosmo is None:
            cp = S.default_cosmo_params()
            cosmo = FlatCosmology(cp.hlittle, cp.OMm)
        cell = float(so.BOX_LEN) / float(so.HII_DIM)
        d_match = cosmo.comoving_distance(float(match_at_z))
        box_size_radians = float(so.BOX_LEN) / d_match
        lon = np.linspace(0, box_size_radians, int(so.HII_DIM))
        lat = np.linspace(0, box_size_radians, int(so.HII_DIM))[::-1]  # x increasing from 0
        LON, LAT = np.meshgrid(lon, lat)
        origin = np.array([0.0, 0.0, -d_match / cell])
        return cls.between_redshifts(min_redshift=match_at_z, max_redshift=max_redshift, resolution=cell,
                                     cosmo=cosmo, latitude=LAT.flatten(), longitude=LON.flatten(), origin=origin,
                                     rotation=LIKE_RECTILINEAR_ROTATION, **kw)

    @property
    def n_pix(self) -> int:
        return len(self.longitude)

    @property
    def nhat(self) -> np.ndarray:
        """The rotated unit directions, float64 (3, n_pix)."""
        if self._nhat is None:
            b, lon = self.latitude, self.longitude
            u = np.stack([np.cos(b) * np.cos(lon), np.cos(b) * np.sin(lon), np.sin(b)])
            self._nhat = np.ascontiguousarray(u if self.rotation is None else self.rotation @ u)
        return self._nhat

    def get_shape(self, simulation_options=None) -> tuple:
        return (self.n_pix, len(self.lc_distances))

    def extended(self, n_low: int, n_high: int) -> "AngularLightconer":
        """This lightconer with ``n_low`` / ``n_high`` more slices at the low- / high-redshift end, spaced
        as its own end slices (the RSD buffer); the directions, origin and rotation are kept."""
        d = self._extended_distances(n_low, n_high)
        if d is None:
            return self
        return AngularLightconer(self.latitude, self.longitude, d, quantities=self.quantities, cosmo=self.cosmo,
                                 interpolation_order=self.interpolation_order, origin=self.origin,
                                 rotation=self.rotation, interp_kinds=self.interp_kinds)

    def angular_tables(self, z_lo, z_hi, cell_size):
        """The slices between the nodes at ``z_lo`` < ``z_hi``: (i0, distance, w_lo, w_hi, w_norm) in
        pixels of ``cell_size`` [Mpc], or None (the selection and weights of the rectilinear lightconer)."""
        pair = self.pair_slices(z_lo, z_hi, cell_size)
        if pair is None:
            return None
        idx, lcd, w_lo, w_hi, w_norm = pair
        return int(idx[0]), lcd, w_lo, w_hi, w_norm

    def validate_options(self, inputs, include_dvdr_in_tau21: bool, apply_rsds: bool):
        """The angular part of validate_options (lightconers.py:678-701): the dv/dr correction and the
        RSDs need the projected velocity, so the 3-D velocities; so does a ``los_velocity`` lightcone."""
        if (include_dvdr_in_tau21 or apply_rsds or "los_velocity" in self.quantities) \
                and not inputs.matter_options.KEEP_3D_VELOCITIES:
            raise ValueError("To account for RSDs or velocity corrections in an angular lightcone, you need to set "
                             "matter_options.KEEP_3D_VELOCITIES=True")
        if self.interpolation_order >= 3:
            mm = sorted(q for q in self.quantities if self.interp_kinds.get(q, "mean") == "mean_max")
            if mm:
                raise ValueError(f"{mm} interpolate with 'mean_max', which needs interpolation_order 0 or 1: "
                                 "spline coefficients of a mean_max interpolation are not built")

    def __eq__(self, other):
        if not isinstance(other, AngularLightconer):
            return NotImplemented

        def close(a, b):
            return a.shape == b.shape and np.allclose(a, b)

        if (self.rotation is None) != (other.rotation is None):
            return False
        return (close(self.latitude, other.latitude) and close(self.longitude, other.longitude)
                and close(self.origin, other.origin) and close(self.lc_distances, other.lc_distances)
                and (self.rotation is None or np.allclose(self.rotation, other.rotation))
                and self.interpolation_order == other.interpolation_order
                and self.quantities == other.quantities and self.interp_kinds == other.interp_kinds
                and (self.cosmo.h, self.cosmo.Om0) == (other.cosmo.h, other.cosmo.Om0))

    __hash__ = None


def lightcone_fields(inputs: Inputs) -> set:
    """Names of the (HII_DIM, HII_DIM, HII_D_PARA) fields a run with these inputs produces per node,
    plus ``los_velocity`` (the line-of-sight velocity: ``velocity_z`` of a rectilinear lightcone, the
    projection of the 3-D velocity of an angular one).  KEEP_3D_VELOCITIES adds ``velocity_x`` /
    ``velocity_y``."""
    mo, ao = inputs.matter_options, inputs.astro_options
    lagrangian, ts_on, mini = mo.SOURCE_MODEL >= 2, bool(ao.USE_TS_FLUCT), bool(ao.USE_MINI_HALOS)
    out = {"density", "velocity_z", "los_velocity", "brightness_temp"} | set(ION_FIELDS)
    if mo.KEEP_3D_VELOCITIES:
        out |= {"velocity_x", "velocity_y"}
    if mo.MINIMIZE_MEMORY:
        out -= {"kinetic_temperature", "mean_free_path"}
    if ao.RECOMB_MODEL == 0:
        out.discard("cumulative_recombinations")
    if mini and not lagrangian:  # one grid per radius
        out.discard("unnormalised_nion")
    if ts_on:
        out |= set(TS_FIELDS) | {"tau_21"} | ({"J_21_LW"} if mini else set())
    if lagrangian:
        out |= {"n_ion", "halo_sfr"} | ({"halo_xray"} if ts_on else set())
        out |= ({"whalo_sfr"} if ao.RECOMB_MODEL else set()) | ({"halo_sfr_mini"} if mini else set())
    return out


def run_lightcone(inputs: Inputs, lightconer, node_redshifts, *, data_path=None,
                  device=None, lib=None, include_dvdr_in_tau21=True, apply_rsds=False, n_rsd_subcells=4,
                  rsd_buffer_slices=(0, 0), halo_catalogs=None, progress=None, keep_perturbed_halos=False):
    """Evolve the node boxes as ``run_coeval`` does and assemble a rectilinear lightcone between
    every pair of nodes on the MI355X (generate_lightcone, drivers/lightcone.py:544-575,596-720).
    Unlike ``run_coeval`` every node is the next one's "previous" snapshot, with or without
    evolution (coeval.py:878-884).  With ``include_dvdr_in_tau21`` (the reference's default) the
    ``brightness_temp`` lightcone is corrected by the line-of-sight velocity gradient at the end
    (rsds.py:16-103): the ``los_velocity`` (and, with USE_TS_FLUCT, ``tau_21``) lightcones are built
    for it and returned too.

    ``apply_rsds`` adds ``<quantity>_with_rsds`` for every lightcone, ``los_velocity`` (and ``tau_21``)
    included: each moved along the line of sight by its peculiar velocity on ``n_rsd_subcells``
    sub-cells per slice, without periodicity, after the dv/dr correction (rsds.py:106-255,
    drivers/lightcone.py:279-303).  The lightcone is then built ``rsd_buffer_slices`` = (low-z,
    high-z) slices longer, as wide as its end slices, and every lightcone is trimmed back to the
    requested distances afterwards; mass moved past the extended ends is lost.  The reference sizes
    that buffer from CLASS's v_b rms, which is not available here: the caller chooses it.

    ``lightconer``: a RectilinearLightconer or an AngularLightconer.  An angular lightcone samples the
    node boxes at its directions with the interpolation order of its lightconer (orders 3 and 5 on the
    B-spline coefficients of every node box, prefiltered once per node); its ``los_velocity`` is the
    3-D velocity projected on the direction, so dv/dr and RSDs need KEEP_3D_VELOCITIES (the reference's
    validate_options, lightconers.py:678-701).  dv/dr and RSDs then act on its (n_pix, n_slices) columns.

    ``device="cuda"`` keeps node boxes and lightcones in HBM; None returns numpy arrays built by the
    same kernels.  Returns a dict: ``lightcones`` {quantity: (HII_DIM, HII_DIM, n_slices) or, angular,
    (n_pix, n_slices)}, ``lightcone_distances`` [Mpc], ``lightcone_redshifts``, ``node_redshifts``
    (descending), ``global_quantities`` {quantity: per-node box means (fp64)} and ``history`` as
    run_coeval's; an angular run adds ``latitude`` and ``longitude``.  ``keep_perturbed_halos`` with a
    catalogue source model adds ``perturbed_halos`` {node redshift: PerturbedHalos}.  ``halo_catalogs``: as
    in ``run_coeval`` -- a function of the node redshift, or ``"sample"`` to find and sample the catalogues
    from the initial conditions (``evolve_halos``: every node is the descendant of the next one up)."""
    so, ao, cp = inputs.simulation_options, inputs.astro_options, inputs.cosmo_params
    angular = isinstance(lightconer, AngularLightconer)
    if not (angular or isinstance(lightconer, RectilinearLightconer)):
        raise TypeError("lightconer must be a RectilinearLightconer or an AngularLightconer")
    nodes64 = sorted((float(z) for z in node_redshifts), reverse=True)
    if len(nodes64) < 2:
        raise ValueError("a lightcone needs at least two node redshifts")
    if len(set(np.float32(nodes64))) != len(nodes64):
        raise ValueError("node redshifts must be distinct")
    if not isinstance(n_rsd_subcells, (int, np.integer)) or isinstance(n_rsd_subcells, bool):
        raise ValueError("n_rsd_subcells must be an integer")
    if apply_rsds and n_rsd_subcells < 1:
        raise ValueError("n_rsd_subcells must be at least 1")
    buf = tuple(int(b) for b in rsd_buffer_slices)
    if len(buf) != 2 or min(buf) < 0:
        raise ValueError("rsd_buffer_slices must be two counts >= 0 (low-z, high-z)")
    requested = lightconer
    if apply_rsds:
        lightconer = lightconer.extended(*buf)
    else:
        buf = (0, 0)
    cosmo = lightconer.cosmo
    if not (math.isclose(cosmo.h, cp.hlittle, rel_tol=1e-12) and math.isclose(cosmo.Om0, cp.OMm, rel_tol=1e-12)):
        raise ValueError("the lightconer's cosmology is not the one of the input parameters")
    lcd = lightconer.lc_distances
    d_node_min, d_node_max = cosmo.comoving_distance(nodes64[-1]), cosmo.comoving_distance(nodes64[0])
    if not (d_node_min <= lcd.min() and lcd.max() <= d_node_max):
        lcz = lightconer.lc_redshifts
        raise ValueError(f"the lightcone ({lcz.min():.4f} .. {lcz.max():.4f}) is not inside the node "
                         f"redshifts ({nodes64[-1]} .. {nodes64[0]}); extend the node redshifts")
    produced = lightcone_fields(inputs)
    unknown = [q for q in lightconer.quantities if q not in produced]
    if unknown:
        raise ValueError(f"{unknown} are not computed for these inputs; possible: {sorted(produced)}")
    if angular:
        lightconer.validate_options(inputs, include_dvdr_in_tau21, apply_rsds)
    quantities = list(dict.fromkeys(lightconer.quantities))
    if include_dvdr_in_tau21:
        if "brightness_temp" not in quantities:
            raise ValueError("include_dvdr_in_tau21 corrects the brightness_temp lightcone: request it")
        if ao.USE_TS_FLUCT and "tau_21" not in quantities:
            quantities.append("tau_21")
        if "los_velocity" not in quantities:
            quantities.append("los_velocity")
    if apply_rsds:
        if lightconer.lc_distances.size < 2:
            raise ValueError("apply_rsds needs a lightcone of at least 2 slices")
        if "los_velocity" not in quantities:
            quantities.append("los_velocity")
    lib = lib or load(require_gpu=True)
    from . import grid_api as api

    los = ("velocity_x", "velocity_y", "velocity_z") if angular else "velocity_z"
    source = {q: (los if q == "los_velocity" else q) for q in quantities}
    n, d_para = int(so.HII_DIM), int(so.NON_CUBIC_FACTOR * so.HII_DIM)
    shape, cell = lightconer.get_shape(so), float(so.BOX_LEN) / float(so.HII_DIM)
    mean_max = tuple(q for q in quantities
                     if q != "los_velocity" and lightconer.interp_kinds.get(source[q], "mean") == "mean_max")
    order = lightconer.interpolation_order if angular else None
    if device is not None:
        import torch

        lcs = {q: torch.zeros(shape, dtype=torch.float32, device=device) for q in quantities}

        def mean(a):
            return float(a.double().mean())

        def full(a):
            return a if tuple(a.shape) == (n, n, d_para) else a.expand(n, n, d_para).contiguous()
    else:
        lcs = {q: np.zeros(shape, np.float32) for q in quantities}

        def mean(a):
            return float(a.mean(dtype=np.float64))

        def full(a):
            return a if a.shape == (n, n, d_para) else np.ascontiguousarray(np.broadcast_to(a, (n, n, d_para)))

    if angular:  # the directions stay where the lightcones are built
        nhat = lightconer.nhat
        if device is not None:
            nhat = torch.from_numpy(nhat).to(device)
        boxes_needed = list(dict.fromkeys(b for q in quantities for b in
                                          (source[q] if isinstance(source[q], tuple) else (source[q],))))

    def node_boxes(boxes):
        """this node's boxes of every lightcone: B-spline coefficients for orders 3 and 5"""
        if not angular:
            return {q: full(boxes[source[q]]) for q in quantities}
        src = {b: full(boxes[b]) for b in boxes_needed}
        if order >= 3:
            src = api.spline_prefilter(src, order)
        return {q: (tuple(src[b] for b in source[q]) if isinstance(source[q], tuple) else src[source[q]])
                for q in quantities}

    nodes32 = [float(np.float32(z)) for z in nodes64]
    z64 = dict(zip(nodes32, nodes64))
    glob = {q: np.zeros(len(nodes32)) for q in lightconer.quantities if q != "los_velocity"}
    history = []
    prev, prev_z = None, None
    snaps = _snapshots(inputs, nodes32, set(nodes32), True, data_path=data_path, device=device, lib=lib,
                       progress=progress, halo_catalogs=halo_catalogs, inspect=None, history=history,
                       perturbed_halos=keep_perturbed_halos)
    moved = {}
    for iz, (z, boxes, _ion, _ts, _ics) in enumerate(snaps):
        if "perturbed_halos" in boxes:
            moved[z64[z]] = boxes["perturbed_halos"]
        for q in glob:
            glob[q][iz] = mean(boxes[q])
        cur = node_boxes(boxes)
        if prev is not None and angular:
            tab = lightconer.angular_tables(z64[z], z64[prev_z], cell)
            if tab is not None:
                i0, dist, w_lo, w_hi, w_norm = tab
                api.lightcone_angular(lcs, cur, prev, i0, dist, w_lo, w_hi, w_norm, nhat, lightconer.origin,
                                      order=order, mean_max=mean_max)
        elif prev is not None:
            tab = lightconer.slab_tables(z64[z], z64[prev_z], cell, d_para)
            if tab is not None:
                i0, plane, w_lo, w_hi, w_norm = tab
                api.lightcone_slices(lcs, cur, prev, i0, plane, w_lo, w_hi, w_norm, mean_max=mean_max)
        prev, prev_z = cur, z
    lcz = lightconer.lc_redshifts
    hubble = cosmo.H0_cgs * cosmo.efunc(lcz)
    if include_dvdr_in_tau21:  # _finalize_lightcone_at_last_redshift (drivers/lightcone.py:265-277)
        api.lightcone_dvdr(lcs["brightness_temp"], lcs["los_velocity"], hubble, cell,
                           float(inputs.astro_params.MAX_DVDR),
                           tau_21=lcs["tau_21"] if ao.USE_TS_FLUCT else None)
    if apply_rsds:  # drivers/lightcone.py:279-303: every quantity, shifted by the unshifted velocity
        shifted = {q + "_with_rsds": (torch.zeros(shape, dtype=torch.float32, device=device) if device is not None
                                      else np.zeros(shape, np.float32)) for q in quantities}
        api.rsd_shift({q: lcs[q] for q in quantities}, lcs["los_velocity"], 1.0 / (hubble * cell),
                      n_sub=int(n_rsd_subcells), periodic=False,
                      out={q: shifted[q + "_with_rsds"] for q in quantities})
        lcs.update(shifted)
    if buf != (0, 0):  # trim (drivers/lightcone.py:303-317)
        keep = slice(buf[0], buf[0] + len(requested.lc_distances))
        lcs = {k: (v[..., keep].contiguous() if device is not None else np.ascontiguousarray(v[..., keep]))
               for k, v in lcs.items()}
        lcd, lcz = lcd[keep], requested.lc_redshifts
    out = {"lightcones": lcs, "lightcone_distances": lcd.copy(), "lightcone_redshifts": lcz,
           "node_redshifts": tuple(nodes64), "global_quantities": glob, "history": history}
    if angular:
        out["latitude"], out["longitude"] = requested.latitude.copy(), requested.longitude.copy()
    if keep_perturbed_halos and moved:
        out["perturbed_halos"] = moved
    return out
