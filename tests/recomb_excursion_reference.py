"""The radius loop of ComputeIonizedBox WITH a recombination model in plain numpy float64, cell by cell:
tests/excursion_reference.py carried over to recomb_model != 0.

Restated from oracle/oracle_ionize.c :405-672 (prepare_box, the filters, the clips :492-501, the barrier
:612-622, Gamma_12 and the mean free path at a first crossing :624-635, z_reion :636-642, the partial
ionisation :649-669), :704-733 (set_recombination_rates) and :257-282 (the splined rate).  Grids are float64,
scalars are narrowed where C holds them in `float`, and the float32 chain runs beside it for E32, exactly as
in excursion_reference.py, whose transforms, crossing bookkeeping, FACTOR and caps this module reuses.

The MARGIN of a cell at a radius is

    m = f zeta - (1 - x_e) (1 + rec),    rec = N / (1 + dens),    the barrier (:621) is m > 0,

with N the cell's previous cumulative_recombinations (CELL_RECOMB, inhomogeneous), element 0 of it
(homogeneous) or the previous N_rec grid filtered with hii_filter and clipped at 0 (CELL_RECOMB off), and dens
the unfiltered, unclipped density x photoncons_adjustment_factor at radius 0, else the filtered delta after
its clips.  Gamma_12 at radius r is R[r] gamma_prefactor / (1 + dens) x the filtered whalo_sfr (Lagrangian;
whalo_sfr filtered like n_ion) or R[r] gamma_prefactor x the mean-fixed f_coll (Eulerian).

E32 (reference side only): `margin` and `mean` as in excursion_reference.py; `gamma`, the largest
|G32 - G64| / G64 at equal radius over the radius-decided crossing cells, G32 rounded to float as a box holds
it; `gamma_abs`, the largest |G32 - G64| over the same cells as a fraction of the largest G64.

Undecided cells: excursion_reference.py grants the two candidates (first crossing under m > +t, under m > -t).
On boxes of 4 M cells that is one candidate short on a handful of cells -- a radius between the two whose
margin lies within t of the barrier as well, where a correct float32 loop may first cross -- and numpy's own
float32 chain takes it (one cell on r1, one on r3).  Restatement.between names those cells and radii, with
their Gamma_12; nothing else is granted.

check_recomb_outputs() is the accounting; what it holds is listed in its docstring.  RestatedCase /
restated() compute a box once per process: test_excursion_reference_host.py and test_gpu_recomb_cells.py share
them."""

import importlib
import time

import numpy as np

import excursion_reference as X
import window_reference as WR
from excursion_reference import F32, FACTOR, FLAG_CAP, FRACT_FLOAT_ERR, RADIUS_CAP, _cross, _f  # noqa: F401
from recomb_helpers import DZ, LNG_MIN, inputs, ln_gamma_knots, recomb_spec

S = importlib.import_module("21cmfast_amd.structs")

GRIDS = ("neutral_fraction", "z_reion", "ionisation_rate_G12", "mean_free_path", "cumulative_recombinations")


# ---------------------------------------------------------------------------------------------- the rate

def rr_rows(z_eff):
    """Table row of oracle_splined_recombination_rate (:260-265), and where z_eff / 0.2f + 0.5 lies within
    1e-9 of an integer -- there the last bit of a libm pow decides the row."""
    z_eff = np.asarray(z_eff, np.float64)
    v = np.where(z_eff > 0, np.minimum(z_eff, 1e6) / DZ + 0.5, 0.0)  # NaN -> row 0
    edge = (z_eff > 0) & (np.abs(v - np.rint(v)) < 1e-9)
    return np.clip(np.floor(v).astype(np.int64), 0, S.RR_NZ - 1), edge


def rr_spline(rr_y, rr_c, z_eff, gamma, row_shift=0):
    """oracle_splined_recombination_rate in numpy float64: row z_ct (+ row_shift, for a test that corrupts
    it), 0 below the ln Gamma floor, the ceiling pulled FRACT_FLOAT_ERR inside, the interval found among the
    knots the C forms with a float step, and gsl's cspline form (b, d from the c coefficients, Horner)."""
    gamma = np.asarray(gamma, np.float64)
    z_ct = np.clip(rr_rows(z_eff)[0] + row_shift, 0, S.RR_NZ - 1)
    knots = ln_gamma_knots()
    top = knots[-1]
    with np.errstate(divide="ignore"):
        lnG = np.log(gamma)
    assert not np.isnan(lnG).any()
    zero = lnG < LNG_MIN
    lnG = np.where(zero, LNG_MIN, np.where(lnG >= top, top - FRACT_FLOAT_ERR, lnG))
    i = np.clip(np.searchsorted(knots, lnG, side="right") - 1, 0, S.RR_NGAMMA - 2)  # knot[i] <= lnG < knot[i+1]
    y0, y1, c0, c1 = rr_y[z_ct, i], rr_y[z_ct, i + 1], rr_c[z_ct, i], rr_c[z_ct, i + 1]
    x_lo = knots[i]
    dx = knots[i + 1] - x_lo
    b = ((y1 - y0) / dx) - dx * (c1 + 2.0 * c0) / 3.0
    d = (c1 - c0) / (3.0 * dx)
    delx = lnG - x_lo
    return np.where(zero, 0.0, y0 + delx * (b + delx * (c0 + delx * d)))


def ln_gamma_edge(gamma):
    """Where ln Gamma lies within 1e-12 relative of the table's floor or top (a libm log decides the branch)."""
    top = ln_gamma_knots()[-1]
    with np.errstate(divide="ignore"):
        lnG = np.log(np.asarray(gamma, np.float64))
    return (np.abs(lnG - LNG_MIN) <= 1e-12 * abs(LNG_MIN)) | (np.abs(lnG - top) <= 1e-12 * abs(top))


# -------------------------------------------------------------------------------------------- the inputs

class Inputs:
    """The float32 input grids of a recombination run (recomb_helpers.inputs), read only."""

    def __init__(self, d, lagrangian, ts):
        self.density, self.prev_nrec, self.prev_z_reion = d["density"], d["prev_nrec"], d["prev_z_reion"]
        self.n_ion = d["n_ion"] if lagrangian else None
        self.whalo_sfr = d["whalo_sfr"] if lagrangian else None
        self.xe = d["xe"] if ts else None
        self.Tneutral = d["Tneutral"] if ts else None
        for a in self.kwargs().values():
            assert a.dtype == F32
            a.setflags(write=False)
        self.density.setflags(write=False)

    def kwargs(self):
        """Everything but the density, as the drivers' keyword arguments."""
        kw = dict(prev_nrec=self.prev_nrec, prev_z_reion=self.prev_z_reion)
        if self.n_ion is not None:
            kw.update(n_ion=self.n_ion, whalo_sfr=self.whalo_sfr)
        if self.xe is not None:
            kw.update(xe=self.xe, Tneutral=self.Tneutral)
        return kw


def _supported(spec, inp):
    lag = spec.fcoll_mode == X.FCOLL_STARS
    assert lag or spec.fcoll_mode == X.FCOLL_ERFC
    assert spec.recomb_model in (1, 2) and (spec.cell_recomb or spec.recomb_model == 2)
    assert not (spec.use_mini_halos or spec.ionise_entire_sphere or spec.r_lowest or spec.first_snapshot)
    assert bool(spec.use_ts_fluct) == (inp.xe is not None) and (inp.n_ion is not None) == lag
    assert inp.density.shape == (spec.hii_dim, spec.hii_dim, spec.hii_dim_z)
    assert inp.prev_nrec.shape == (inp.density.shape if spec.recomb_model == 2 else (1, 1, 1))
    return lag


class _Chain:
    """One precision of the loop: the unfiltered spectra, and per radius the margin and Gamma_12 grids."""

    def __init__(self, spec, inp, f32, round_trip0=None):
        self.spec, self.inp, self.f32 = spec, inp, f32
        self.round_trip0 = round_trip0 if f32 else None
        self.lag = _supported(spec, inp)
        self.filter_rec = not spec.cell_recomb
        self.real = F32 if f32 else np.float64
        self.shape = inp.density.shape
        self.raw_dens = inp.density.astype(np.float64) * spec.photoncons_adjustment_factor
        self.grids = {"delta": np.clip(self.raw_dens, -1.0, 1e6)}  # prepare_box, :406-411
        if self.lag:
            self.grids["stars"] = np.clip(inp.n_ion.astype(np.float64), 0.0, 1e20)
            self.grids["sfr"] = np.clip(inp.whalo_sfr.astype(np.float64), 0.0, 1e20)
        if inp.xe is not None:
            self.grids["xe"] = np.clip(inp.xe.astype(np.float64), 0.0, 1.0)
        if self.filter_rec:
            self.grids["nrec"] = np.clip(inp.prev_nrec.astype(np.float64), 0.0, 1e20)
        self.spectra = {k: X._rfftn(g.astype(self.real)) for k, g in self.grids.items()}
        assert all(A.dtype == (np.complex64 if f32 else np.complex128) for A in self.spectra.values())
        # :613-616: the previous count as it is, no clip
        self.cell_nrec = None
        if spec.cell_recomb:
            self.cell_nrec = inp.prev_nrec.astype(np.float64) if spec.recomb_model == 2 else float(inp.prev_nrec.ravel()[0])

    def filtered(self, name, r, W):
        """copy_filter_c2r; radius 0 takes the clipped input, as excursion_reference._Chain.filtered does --
        unless this is the float32 chain of an oracle pin, which sends it through the float32 transform pair
        `round_trip0` as the oracle does (:308-315)."""
        if r == 0:
            g = self.grids[name]
            return g if self.round_trip0 is None else self.round_trip0(g.astype(F32)).astype(np.float64)
        g = X._irfftn(self.spectra[name] * W.astype(self.real), self.shape)
        assert g.dtype == self.real
        return g.astype(np.float64)

    def radius(self, r, W_hii, W_stars):
        """(margin, f_coll_grid_mean after the floor, f zeta, x_e, Gamma_12) of radius index r: double
        expressions of the (float or double) grids, as the oracle's per-cell arithmetic is."""
        s = self.spec
        delta = self.filtered("delta", r, W_hii)
        if not self.lag:
            delta = np.clip(delta, -1.0, 1e6)  # clip_and_get_extrema, :438-448
        delta = np.maximum(delta, _f(-1.0 + FRACT_FLOAT_ERR) if self.f32 else -1.0 + FRACT_FLOAT_ERR)  # :492
        if self.lag:
            f = np.maximum(self.filtered("stars", r, W_stars), 0.0)  # :500
            sfr = np.maximum(self.filtered("sfr", r, W_stars), 0.0)  # :501
        else:
            f = X.fgtrm_bias_fast(s, r, delta, self.f32)  # :547-549, stored as float at :556
        mean = float(f.sum(dtype=np.float64)) / f.size
        mean = max(mean, s.f_limit_acg if s.mass_dep_zeta else FRACT_FLOAT_ERR)  # :573-578
        if s.fix_mean:
            f = (s.mean_f_coll / mean) * f  # :586, :602
        dens = self.raw_dens if r == 0 else delta  # :594-597
        if self.lag:
            f = f * (1 / (s.rhocrit_omb * (1 + dens)))  # :603
        if s.mass_dep_zeta:
            f = np.maximum(f, s.f_limit_acg)  # :608
        fz = f * s.ion_eff_factor
        if self.filter_rec:
            rec = np.maximum(self.filtered("nrec", r, W_hii), 0.0) / (1.0 + dens)  # :493, :616-617
        else:
            rec = self.cell_nrec / (1.0 + dens)
        xe = None
        if self.inp.xe is not None:
            xe = np.clip(self.filtered("xe", r, W_hii), 0.0, _f(0.999) if self.f32 else 0.999)  # :495-496
        m = fz - (1.0 - (0.0 if xe is None else xe)) * (1.0 + rec)  # :621-622
        if self.lag:
            gamma = s.R[r] * s.gamma_prefactor / (1 + dens) * sfr  # :626-627
        else:
            gamma = s.R[r] * (s.gamma_prefactor * f)  # :629-632
        return m, mean, fz, xe, gamma


def radius_loop(spec, inp, with_f32=False, round_trip0=None):
    """Radius indices from the largest down to 0: yields (r, float64 results, float32 results or None)."""
    c64 = _Chain(spec, inp, False)
    c32 = _Chain(spec, inp, True, round_trip0) if with_f32 else None
    k = WR.k_magnitude(c64.shape, spec.box_len, spec.box_len_z)
    for r in range(spec.n_radii - 1, -1, -1):
        W_hii = W_stars = None
        if r > 0:
            W_hii = WR.window(spec.hii_filter, k, spec.R[r], 0.0)
            if c64.lag:
                W_stars = WR.window(spec.stars_filter, k, spec.R[r], spec.mfp_meandens)
        yield r, c64.radius(r, W_hii, W_stars), (c32.radius(r, W_hii, W_stars) if c32 else None)


# ----------------------------------------------------------------------------- set_recombination_rates

class Rates:
    """What :704-733 reads beside the box's own Gamma_12 and x_HI."""

    def __init__(self, spec, inp):
        self.rr_y, self.rr_c = spec._rr
        self.inhomo = spec.recomb_model == 2
        self.stored_redshift, self.scale = spec.stored_redshift, (spec.fabs_dtdz, spec.dz)
        self.density, self.prev_nrec = inp.density, inp.prev_nrec

    def z_eff(self):
        return (1.0 + self.density.astype(np.float64)) ** (1.0 / 3.0) * (1 + self.stored_redshift) - 1.0  # :721-725

    def cells(self, G12, xhi, row_shift=0):
        """:718-731 in float64 from float Gamma_12 and x_HI grids, before the store narrows it."""
        rate = rr_spline(self.rr_y, self.rr_c, self.z_eff(), G12.astype(np.float64), row_shift)
        return self.prev_nrec.astype(np.float64) + rate * self.scale[0] * self.scale[1] * (1.0 - xhi.astype(np.float64))

    def left_out(self, G12):
        """The cells the 1-ulp comparison leaves out: a row or a table end decided by the last bit of libm."""
        return rr_rows(self.z_eff())[1] | ln_gamma_edge(G12)

    def homogeneous(self, G12, xhi):
        """:705-716.  (value, lowest, highest): the mean Gamma_12 and the global x_HI pass through `float`
        there; lowest / highest span rr_spline over the two float neighbours of each of the two means."""
        ntot = float(F32(G12.size))
        g = F32(float(G12.sum(dtype=np.float64)) / ntot)
        x = F32(float(xhi.sum(dtype=np.float64)) / ntot)
        prev = float(self.prev_nrec.ravel()[0])

        def cum(gg, xx):
            rate = float(rr_spline(self.rr_y, self.rr_c, self.stored_redshift, float(gg)))
            return prev + rate * self.scale[0] * self.scale[1] * (1.0 - float(xx))

        inf = F32(np.inf)
        span = [cum(gg, xx) for gg in (np.nextafter(g, -inf), g, np.nextafter(g, inf))
                for xx in (np.nextafter(x, -inf), x, np.nextafter(x, inf))]
        return cum(g, x), min(span), max(span)


def ulp_distance(a, b):
    """Distance in float32 steps between two non-negative float32 arrays."""
    assert a.dtype == F32 and b.dtype == F32 and (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------- E32

def radii_f32(spec):
    R = np.array([spec.R[i] for i in range(spec.n_radii)], np.float64).astype(F32)
    assert (np.diff(R) > 0).all()
    return R


def mean_free_path_of(cross, R32):
    """The mean_free_path grid of a 1-based crossing index."""
    return np.where(cross > 0, R32[np.maximum(cross.astype(np.int64) - 1, 0)], F32(0)).astype(F32)


def z_reion_of(crossing, prev_z_reion, redshift):
    """:636-642 over :356: the redshift at a crossing unless the cell holds an earlier one, else -1."""
    return np.where(crossing, np.where(prev_z_reion < 0, F32(redshift), prev_z_reion), F32(-1.0)).astype(F32)


def e32(spec, inp, round_trip0=None):
    """The float32 chain beside the float64 one.  `margin`, `mean`: as excursion_reference.e32.  `xhi`: the
    largest deviation of the partial ionisation of radius 0 (restate() uses it for an oracle pin).  `cross0`,
    `G64`, `G32`: the float64 chain's first crossing under m > 0 and both chains' Gamma_12 at THAT radius
    (restate() turns them into `gamma` / `gamma_abs` once it knows the radius-decided cells).  `outputs`: what
    the float32 chain itself gives, in the form check_recomb_outputs() takes."""
    e_m = e_mean = 0.0
    shape = inp.density.shape
    c0, c32 = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    G64, G32, Gout = np.zeros(shape), np.zeros(shape, F32), np.zeros(shape, F32)
    means = np.zeros(spec.n_radii)
    for r, (m64, mean64, fz64, xe64, g64), (m32, mean32, fz32, xe32, g32) in radius_loop(spec, inp, True, round_trip0):
        e_m = max(e_m, float(np.abs(m32 - m64).max()))
        e_mean = max(e_mean, abs(mean32 - mean64) / mean64)
        g32 = g32.astype(F32)  # as a box holds it
        new = (c0 == 0) & (m64 > 0)
        G64[new], G32[new] = g64[new], g32[new]
        c0 = _cross(c0, m64, r, 0.0)
        new = (c32 == 0) & (m32 > 0)
        Gout[new] = g32[new]
        c32 = _cross(c32, m32, r, 0.0)
        means[r] = mean32
    e_xhi = float(np.abs(X.partial_xhi(fz32, xe32) - X.partial_xhi(fz64, xe64)).max())  # radius 0 came last
    xhi = np.where(c32 > 0, 0.0, X.partial_xhi(fz32, xe32)).astype(F32)
    rates = Rates(spec, inp)
    if rates.inhomo:
        nrec = rates.cells(Gout, xhi).astype(F32)
    else:
        nrec = np.full((1, 1, 1), rates.homogeneous(Gout, xhi)[0], F32)
    out = {"neutral_fraction": xhi, "z_reion": z_reion_of(c32 > 0, inp.prev_z_reion, spec.redshift),
           "ionisation_rate_G12": Gout, "mean_free_path": mean_free_path_of(c32, radii_f32(spec)),
           "cumulative_recombinations": nrec, "f_coll_grid_mean": means}
    return {"margin": e_m, "mean": e_mean, "xhi": e_xhi, "cross0": c0, "G64": G64, "G32": G32, "outputs": out}


class Restatement:
    """The float64 loop at tolerance t: everything check_recomb_outputs() holds a set of outputs against."""

    def __init__(self, spec, inp, t, mean_tol):
        self.t, self.mean_tol = t, mean_tol
        self.xhi_tol = self.gamma_rel = self.gamma_abs = None  # restate() fills them
        self.redshift, self.R32, self.prev_z_reion = F32(spec.redshift), radii_f32(spec), inp.prev_z_reion
        self.rates = Rates(spec, inp)
        shape = inp.density.shape
        hi, lo = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)  # first crossing under m > +t, m > -t
        self.G_hi, self.G_lo = np.zeros(shape), np.zeros(shape)  # Gamma_12 at those radii
        self.f_coll_grid_mean = np.zeros(spec.n_radii)
        # Candidates BETWEEN the two: a radius below the -t crossing and above the +t crossing whose margin
        # lies within t of the barrier as well.  A correct float32 loop may first cross there (margins -0.5 t,
        # +0.5 t, 2 t at three successive radii: the middle one is neither the +t nor the -t crossing).
        # (flat cell index, 1-based radius index) -> Gamma_12; a few cells per 4 M-cell box.
        self.between = {}
        for r, (m, mean, fz, xe, g), _ in radius_loop(spec, inp):
            mid = np.flatnonzero((lo > 0) & (hi == 0) & (m > -t) & (m <= t))
            self.between.update({(int(i), r + 1): float(g.reshape(-1)[i]) for i in mid})
            new = (hi == 0) & (m > t)
            self.G_hi[new] = g[new]
            new = (lo == 0) & (m > -t)
            self.G_lo[new] = g[new]
            hi, lo = _cross(hi, m, r, t), _cross(lo, m, r, -t)
            self.f_coll_grid_mean[r] = mean
        self.cross_hi, self.cross_lo = hi, lo
        self.flag_decided = (hi > 0) == (lo > 0)
        self.radius_decided = hi == lo
        self.decided_flag = hi > 0  # where flag_decided
        self.xhi = X.partial_xhi(fz, xe)  # radius 0 came last; no rec term (:650-669)
        flat_hi = hi.reshape(-1)
        self.between = {k: v for k, v in self.between.items() if k[1] > flat_hi[k[0]]}
        for a in (hi, lo, self.G_hi, self.G_lo, self.flag_decided, self.radius_decided, self.xhi):
            a.setflags(write=False)

    @property
    def flag_undecided_share(self):
        return 1.0 - float(self.flag_decided.mean())

    @property
    def radius_undecided_share(self):
        return 1.0 - float(self.radius_decided.mean())

    @property
    def ionised_share(self):
        return float((self.cross_hi > 0).mean())


def restate(spec, inp, round_trip0=None):
    """E32, then the restatement at t = FACTOR * E32.  Returns (Restatement, the dict of e32() with `gamma`
    and `gamma_abs` added and the grids it no longer needs dropped).

    round_trip0 is for holding the ORACLE to the accounting: its radius 0 goes through a float32 transform
    pair, which the library's loops and this module do not make (excursion_reference.py, "Radius 0"); on an
    n_ion grid that moves x_HI by up to 1e-5, and by how much is a property of the transform (the oracle's
    own radix order), not of float32 arithmetic at large.  round_trip0 is that pair as a function of a float32
    grid (the oracle's own forward and inverse transforms); the float32 chain then sends its radius-0 grids
    through it, so that E32 -- margin, Gamma_12 and the partial ionisation of radius 0 alike -- measures a
    float32 implementation of the oracle's kind, and the x_HI bound becomes the larger of the expression's
    bound and FACTOR x that measured deviation.  The float64 side is the same either way."""
    e = e32(spec, inp, round_trip0)
    ref = Restatement(spec, inp, FACTOR * e["margin"], FACTOR * e["mean"])
    ref.xhi_tol = FACTOR * X.xhi_float32_bound(spec, inp, ref.f_coll_grid_mean[0])
    if round_trip0 is not None:
        ref.xhi_tol = max(ref.xhi_tol, FACTOR * e["xhi"])
    sel = ref.radius_decided & (ref.cross_hi > 0)
    assert sel.any() and (e["cross0"][sel] == ref.cross_hi[sel]).all()
    G64, G32 = e.pop("G64")[sel], e.pop("G32")[sel].astype(np.float64)
    del e["cross0"]
    assert (G64 == ref.G_hi[sel]).all()
    ref.gamma_max = float(G64.max())
    diff, pos = np.abs(G32 - G64), G64 > 0
    e["gamma"] = float((diff[pos] / G64[pos]).max())
    e["gamma_abs"] = float(diff.max()) / ref.gamma_max
    ref.gamma_rel, ref.gamma_abs = FACTOR * e["gamma"], FACTOR * e["gamma_abs"] * ref.gamma_max
    return ref, e


# ------------------------------------------------------------------------------------------- accounting

def device_cross(mfp, R32):
    """The 1-based crossing index a mean_free_path grid names: r + 1 where it is float(R[r]) exactly, 0 where
    it is 0; any other value raises."""
    assert mfp.dtype == F32
    idx = np.minimum(np.searchsorted(R32, mfp), len(R32) - 1)
    hit = R32[idx] == mfp
    other = ~hit & (mfp != 0)
    n = int(other.sum())
    assert n == 0, (f"mean_free_path is neither 0 nor one of the radii: {n} cells, first at "
                    f"{np.argwhere(other)[:5].tolist()}, values {mfp[other][:5].tolist()}")
    return np.where(hit, idx + 1, 0).astype(np.int32)


def check_recomb_outputs(ref, out):
    """The cell-by-cell accounting of one set of outputs (the five GRIDS and f_coll_grid_mean).  No share of
    cells is excused beyond the undecided sets that `ref` alone names at t = FACTOR * E32:
      * mean_free_path is 0 or float(R[r]); that names the crossing index (x_HI == 0 does not: a partial
        ionisation clamps to 0 without a crossing);
      * the decided crossing flag on every flag-decided cell; the decided first-crossing radius on every
        radius-decided cell; elsewhere one of the two candidates (the first crossing under m > +t or under
        m > -t) or, on the few cells where `ref` finds one, a radius between the two whose float64 margin lies
        within t of the barrier as well (Restatement.between: with 4 M cells and 5e-4 of them undecided, two
        successive radii within t of the barrier in one cell is an expected event, not a rare one);
      * Gamma_12 == 0 exactly where there is no crossing; at a crossing within FACTOR x E32['gamma'] relative
        plus FACTOR x E32['gamma_abs'] of the largest Gamma_12, against the float64 Gamma_12 of the radius the
        mean free path names;
      * z_reion exactly float(redshift) / the previous z_reion >= 0 / -1, following the crossings;
      * x_HI == 0 at every crossing; on decided non-crossing cells within the radius-0 float32 bound;
      * f_coll_grid_mean[r] within FACTOR x the measured float32 deviation;
      * cumulative_recombinations: recomputed in float64 from the outputs' own Gamma_12 and x_HI, 1 float32
        ulp (inhomogeneous; at most 10 cells left out at a table edge), or within the span of the float
        neighbours of the two means plus 1 ulp (homogeneous).
    Raises AssertionError naming what differs, the count and the first places; returns the figures of the
    RECOMB-EXCURSION line."""
    xhi, zre, G12 = out["neutral_fraction"], out["z_reion"], out["ionisation_rate_G12"]
    nrec = out["cumulative_recombinations"]
    for a in (xhi, zre, G12, out["mean_free_path"], nrec):
        assert a.dtype == F32

    def bad(what, mask):
        n = int(mask.sum())
        assert n == 0, f"{what}: {n} cells, first at {np.argwhere(mask)[:5].tolist()}"

    cross = device_cross(out["mean_free_path"], ref.R32)
    crossing = cross > 0
    hi, lo = ref.cross_hi.astype(np.int32), ref.cross_lo.astype(np.int32)
    bad("decided cells with the wrong crossing flag", ref.flag_decided & (crossing != ref.decided_flag))
    bad("decided cells with the wrong first-crossing radius", ref.radius_decided & (cross != hi))
    third = ~ref.radius_decided & (cross != hi) & (cross != lo)
    between = [(int(i), int(cross.reshape(-1)[i])) for i in np.flatnonzero(third)]
    for k in between:  # a candidate between the two, which the reference names too
        third.reshape(-1)[k[0]] = k not in ref.between
    bad("undecided cells with a first-crossing radius that is no candidate", third)
    # Gamma_12
    bad("Gamma_12 is not 0 on a cell without a crossing", ~crossing & (G12 != 0))
    want = np.where(cross == hi, ref.G_hi, ref.G_lo)  # the previous check left no other radius ...
    for k in between:  # ... but these
        want.reshape(-1)[k[0]] = ref.between[k]
    dev = np.abs(G12.astype(np.float64) - want)
    bound = ref.gamma_rel * want + ref.gamma_abs
    worst = float((dev[crossing] / bound[crossing]).max()) if crossing.any() else 0.0
    bad(f"Gamma_12 at the radius its mean free path names is off by more than {ref.gamma_rel:.3g} relative + "
        f"{ref.gamma_abs:.3g} (largest: {worst:.3g} of the bound)", crossing & (dev > bound))
    # z_reion
    bad("z_reion is not float(redshift) on a crossing cell that held none", crossing & (ref.prev_z_reion < 0)
        & (zre != ref.redshift))
    bad("z_reion is not the previous z_reion on a crossing cell that held one", crossing & (ref.prev_z_reion >= 0)
        & (zre != ref.prev_z_reion))
    bad("z_reion is not -1 on a cell without a crossing", ~crossing & (zre != F32(-1.0)))
    # neutral fraction
    bad("x_HI is not 0 on a crossing cell", crossing & (xhi != 0))
    neutral = ref.flag_decided & ~ref.decided_flag
    xdev = np.abs(xhi.astype(np.float64) - ref.xhi)
    xhi_dev = float(xdev[neutral].max()) if neutral.any() else 0.0
    bad(f"x_HI off by more than {ref.xhi_tol:.3g} on decided non-crossing cells (largest {xhi_dev:.3g})",
        neutral & (xdev > ref.xhi_tol))
    # per-radius means
    means = np.asarray(out["f_coll_grid_mean"], np.float64)
    mean_dev = np.abs(means - ref.f_coll_grid_mean) / ref.f_coll_grid_mean
    r = int(np.argmax(mean_dev))
    assert mean_dev[r] <= ref.mean_tol, (f"f_coll_grid_mean[{r}] = {means[r]!r} against {ref.f_coll_grid_mean[r]!r}: "
                                         f"off by {mean_dev[r]:.3g} relative, bound {ref.mean_tol:.3g}")
    # cumulative recombinations, from the outputs' own Gamma_12 and x_HI
    if ref.rates.inhomo:
        assert nrec.shape == xhi.shape
        skip = ref.rates.left_out(G12)
        assert skip.sum() <= 10, f"{int(skip.sum())} cells at a table edge: the box is no fair test of N_rec"
        ulps = np.where(skip, 0, ulp_distance(nrec, ref.rates.cells(G12, xhi).astype(F32)))
        nrec_ulp = int(ulps.max())
        bad(f"cumulative_recombinations more than 1 float ulp from the float64 rate of the outputs' own "
            f"Gamma_12 and x_HI (largest {nrec_ulp})", ulps > 1)
    else:
        assert nrec.shape == (1, 1, 1)
        got = nrec.ravel()[0]
        value, low, high = ref.rates.homogeneous(G12, xhi)
        inf = F32(np.inf)
        assert np.nextafter(F32(low), -inf) <= got <= np.nextafter(F32(high), inf), (
            f"cumulative_recombinations (homogeneous) = {got!r} outside [{low!r}, {high!r}] + 1 float ulp")
        nrec_ulp = int(ulp_distance(nrec.ravel(), np.full(1, value, F32))[0])
    return {"took_minus_t": int((~ref.radius_decided & (cross == lo)).sum()), "took_between": len(between),
            "mean_dev_over_bound": float(mean_dev[r] / ref.mean_tol), "xhi_dev": xhi_dev,
            "gamma_over_bound": worst, "nrec_ulp": nrec_ulp}


def recomb_line(name, ref, e, fig):
    return (f"RECOMB-EXCURSION {name}: E32 margin {e['margin']:.2e} mean {e['mean']:.2e} gamma {e['gamma']:.2e} "
            f"gamma_abs {e['gamma_abs']:.2e}, flag-undecided {ref.flag_undecided_share:.2e}, radius-undecided "
            f"{ref.radius_undecided_share:.2e}, took the -t candidate on {fig['took_minus_t']} cells and one between on {fig['took_between']} of "
            f"{len(ref.between)}, Gamma_12 "
            f"deviation {fig['gamma_over_bound']:.3f} of its bound, mean deviation "
            f"{fig['mean_dev_over_bound']:.3f} of its bound, x_HI deviation {fig['xhi_dev']:.2e} (bound "
            f"{ref.xhi_tol:.2e}), N_rec within {fig['nrec_ulp']} ulp")


# ------------------------------------------------------------------------------------------- the boxes
#   name: (nx = ny, nz, recomb model, CELL_RECOMB, x_e grid, Lagrangian, r_bubble_max, seed)
# r1 - r4 are the smallest boxes that reach each fused pass-Z kernel (nx >= 128, 256- or 512-point z-lines);
# test_excursion_reference_host.py holds every box to the caps.
CASES = {
    "r1": (128, 256, 2, 1, False, True, 20.0, 77),   # c21hip_split_z_ionise with recomb, dense N_rec rows
    "r2": (128, 256, 2, 0, False, True, 10.0, 77),   # ..._recomb_nrec: the filtered N_rec as third spectrum
    "r3": (128, 256, 1, 1, True, True, 10.0, 77),    # ..._recomb_xe, homogeneous N = 0.25
    "r4": (128, 512, 2, 0, True, True, 8.0, 77),     # ..._recomb_xe_nrec: four spectra
    "u-64": (64, 64, 2, 0, True, True, 10.0, 77),    # native passes, unfused: all five grids in ionise_recomb_kernel
    "u-50": (50, 50, 2, 1, False, True, 11.0, 77),   # the rocFFT route; an even number of radii (26)
    "e-64": (64, 64, 2, 0, False, False, 10.0, 77),  # Eulerian Gamma_12, the mean fix
}
HOMOGENEOUS_NREC = 0.25


def make_case(n, nz, model, cell, ts, lagrangian, r_max, seed):
    spec = recomb_spec(n, model=model, cell_recomb=cell, lagrangian=lagrangian, hii_dim_z=nz, ts=int(ts),
                       r_bubble_max=r_max)
    d = inputs((n, n, nz), seed=seed, ts=ts)
    if model == 1:
        d["prev_nrec"] = np.full((1, 1, 1), HOMOGENEOUS_NREC, F32)
    return spec, Inputs(d, lagrangian, ts)


class RestatedCase:
    def __init__(self, key, round_trip0=None):
        t0 = time.perf_counter()
        self.spec, self.inp = make_case(*CASES.get(key, key))
        self.ref, self.e = restate(self.spec, self.inp, round_trip0)
        self.host_seconds = time.perf_counter() - t0


_restated = {}


def restated(key, round_trip0=None):
    """A box of CASES (by name) or any make_case() tuple, restated once per process; read only."""
    if (key, round_trip0 is not None) not in _restated:
        _restated[key, round_trip0 is not None] = RestatedCase(key, round_trip0)
    return _restated[key, round_trip0 is not None]


def caps_line(name, c):
    n, nz, model, cell, ts, lag, r_max, seed = CASES.get(name, name)
    return (f"RECOMB-CAPS {name}: {n}x{n}x{nz} model {model} CELL_RECOMB {cell} x_e {'yes' if ts else 'no'} "
            f"{'Lagrangian' if lag else 'Eulerian'} r_bubble_max {r_max:g} seed {seed} n_radii {c.spec.n_radii}, "
            f"E32 margin {c.e['margin']:.2e}, flag-undecided {c.ref.flag_undecided_share:.2e}, radius-undecided "
            f"{c.ref.radius_undecided_share:.2e}, ionised {c.ref.ionised_share:.2f}, crossings at "
            f"{len(np.unique(c.ref.cross_hi)) - 1} radii, host {c.host_seconds:.0f} s")
