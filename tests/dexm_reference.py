"""The DexM halo finder restated serially in numpy (reference: HaloCatalog.c:155-358, check_halo, pixel_in_halo)
for tests/test_gpu_dexm.py and tests/test_dexm_host.py: the radius ladder, the raster-order greedy selection on
given filtered fields, the catalogue rows with their Philox deviates, and the overlap box in float64.

check_halo's arithmetic is kept: R and BOX_LEN are floats, so R / BOX_LEN * DIM is a float32 quotient; its
ceiling is the search range, its float64 square rounded to float32 the strict bound on the float32 squared
distance to the nearest of the 27 periodic images.  A cell with a smaller squared distance than that bound is
always inside the search range, so a sphere is the set of cells {bound > distance^2} (as long as the range
is below the box size, where the reference's single wrap is valid)."""

import math

import numpy as np

import halo_sampler_reference as HS
import window_reference as WR

F32 = np.float32
L_FACTOR = 0.620350491
DRAW_DEXM = 8


def ladder(host, so, sampler, redshift):
    """HaloCatalog.c:81-200 with the reference's float variables: [(R, M, delta_crit)] of the kept rungs and
    the number skipped as rarer than 7 sigma.  `host`: the library with dicke / sigma_z0 / c21_RtoM / c21_MtoR
    declared as double functions."""
    growth = F32(host.dicke(redshift))
    m_min = F32(host.c21_RtoM(L_FACTOR * so.BOX_LEN / (so.HII_DIM if sampler else so.DIM)))
    delta_r = F32(L_FACTOR * 2.0 * so.BOX_LEN / so.DIM)
    R = F32(host.c21_MtoR(float(m_min) * 1.01))
    while R < L_FACTOR * so.BOX_LEN:
        R = F32(float(R) * so.DELTA_R_FACTOR)
    kept, skipped = [], 0
    while R > 0.5 * float(delta_r) and host.c21_RtoM(float(R)) >= float(m_min):
        M = F32(host.c21_RtoM(float(R)))
        sig, dl = host.sigma_z0(float(M)), 1.686 / float(growth)
        dcrit = F32(float(growth) * (math.sqrt(0.73) * dl * (1.0 + 0.15 * (sig * sig / (0.73 * dl * dl)) ** 0.05)))
        if sig * float(growth) * 7.0 < float(dcrit):
            skipped += 1
        else:
            kept.append((R, M, dcrit))
        R = F32(float(R) / so.DELTA_R_FACTOR)
    return kept, skipped, growth


class Finder:
    """The serial finder on a box [dim][dim][dim_z] (z fastest)."""

    def __init__(self, dim, dim_z, box_len, r_overlap=1.0, optimize=False, optimize_minmass=0.0, rtom_unit=1.0):
        self.n, self.nz = int(dim), int(dim_z)
        self.box_len = F32(box_len)
        self.r_overlap, self.optimize, self.minmass = float(r_overlap), bool(optimize), float(optimize_minmass)
        self.rtom_unit = float(rtom_unit)
        self._cache = {}

    def sphere(self, R):
        """offsets (ox, oy, oz) of the cells of a sphere of float radius R around a centre, and its range"""
        R = F32(R)
        key = R.tobytes()
        if key not in self._cache:
            q = F32(F32(R / self.box_len) * F32(self.n))
            r_index = int(math.ceil(float(q)))
            assert r_index < min(self.n, self.nz), "the reference's single wrap needs R_index < DIM"
            rsq = F32(float(q) * float(q))

            def axis(n):
                d = np.arange(n)
                m = np.minimum(d, n - d).astype(F32)
                return m * m

            xs, zs = axis(self.n), axis(self.nz)
            dist = (xs[:, None, None] + xs[None, :, None]) + zs[None, None, :]
            assert dist.dtype == F32
            ox, oy, oz = np.nonzero(rsq > dist)
            self._cache[key] = (ox, oy, oz, r_index)
        return self._cache[key]

    def cells(self, cell, sph):
        n, nz = self.n, self.nz
        z, t = cell % nz, cell // nz
        y, x = t % n, t // n
        return (((x + sph[0]) % n) * n + (y + sph[1]) % n) * nz + (z + sph[2]) % nz

    def run(self, filtered, R, mass, delta_crit):
        """filtered [n_R][N] float32 (delta_m of every rung); returns (in_halo uint8 [N], rung of the halo
        centred on each cell or -1 [N], halos per rung, candidates over the threshold per rung)"""
        n_cells = self.n * self.n * self.nz
        in_halo = np.zeros(n_cells, np.uint8)
        forbidden = np.zeros(n_cells, np.uint8)
        rung_of = np.full(n_cells, -1, np.int32)
        found, per_rung, over = [], [], []
        for r in range(len(R)):
            Rr, M = F32(R[r]), F32(mass[r])
            cand = np.flatnonzero(np.asarray(filtered[r], F32).ravel() > F32(delta_crit[r]))
            over.append(cand.size)
            paint = self.sphere(Rr)
            test = self.sphere(F32(float(Rr) * self.r_overlap))  # R *= DEXM_R_OVERLAP (a double)
            opt = self.optimize and float(M) > self.minmass
            count = 0
            if opt:
                grow = self.sphere(F32((1.0 + self.r_overlap) * float(Rr)))
                forbidden[:] = 0
                for cell in found:  # MtoR(M_h) as a float, + DEXM_R_OVERLAP * R in double, passed as a float
                    r_h = F32((float(mass[rung_of[cell]]) / self.rtom_unit) ** (1.0 / 3.0))
                    forbidden[self.cells(cell, self.sphere(F32(float(r_h) + self.r_overlap * float(Rr))))] = 1
            for cell in cand:
                if opt:
                    if forbidden[cell]:
                        continue
                    forbidden[self.cells(cell, grow)] = 1
                else:
                    if in_halo[cell] or in_halo[self.cells(cell, test)].any():
                        continue
                in_halo[self.cells(cell, paint)] = 1
                rung_of[cell] = r
                found.append(int(cell))
                count += 1
            per_rung.append(count)
        return in_halo, rung_of, per_rung, over

    def catalogue(self, rung_of, mass, seed, redshift):
        """the rows in raster order: masses, coordinates x * (BOX_LEN / DIM) with the float quotient, and the
        three deviates of one Philox block per halo (four 32-bit uniforms, Box-Muller on (u0, u1) and (u2, u3))"""
        cells = np.flatnonzero(rung_of >= 0)
        nz, n = self.nz, self.n
        idx = np.stack([cells // (nz * n), (cells // nz) % n, cells % nz], axis=1)
        cell_length = float(F32(self.box_len / F32(n)))
        key = (int(seed) + int(redshift * 1000)) & 0xFFFFFFFFFFFFFFFF
        c = cells.astype(np.uint64)
        w = HS.philox(np.uint64(0), np.uint64(DRAW_DEXM), c & HS.U32, c >> np.uint64(32), key)
        u = [(x.astype(np.float64) + 0.5) * 2.0 ** -32 for x in w]
        ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
        return dict(halo_masses=np.asarray(mass, F32)[rung_of[cells]],
                    halo_coords=(idx * cell_length).astype(F32),
                    star_rng=(ra * np.cos(2.0 * np.pi * u[1])).astype(F32),
                    sfr_rng=(ra * np.sin(2.0 * np.pi * u[1])).astype(F32),
                    xray_rng=(rb * np.cos(2.0 * np.pi * u[3])).astype(F32))


def filtered_f64(density, box_len, box_len_z, halo_filter, R, growth):
    """the float64 filter of the hi-res density at the radii R, times the growth factor: [n_R][shape]"""
    a = np.asarray(density, np.float64)
    spectrum = np.fft.rfftn(a)
    k = WR.k_magnitude(a.shape, box_len, box_len_z)
    return np.stack([np.fft.irfftn(WR.filtered_spectrum(a, box_len, box_len_z, halo_filter, float(r), spectrum=spectrum,
                                                        k=k), s=a.shape, axes=(0, 1, 2)) * float(growth) for r in R])


def overlap_f64(in_halo, box_len, box_len_z, hii_dim, hii_dim_z):
    """HaloCatalog.c:361-420 in float64: the 0 / 1 mask smoothed with the real-space top-hat of the low-res
    cell (when the grids differ), sampled at (int)(i * DIM / (float)HII_DIM + 0.5), clamped to [0, 1]"""
    a = np.asarray(in_halo, np.float64)
    dim, dim_z = a.shape[0], a.shape[2]
    if dim != hii_dim:
        R = F32(L_FACTOR * float(F32(box_len)) / hii_dim)
        a = np.fft.irfftn(WR.filtered_spectrum(a, box_len, box_len_z, 0, float(R)), s=a.shape, axes=(0, 1, 2))
    f = F32(dim) / F32(hii_dim)

    def pick(m, top):
        return np.minimum((np.arange(m).astype(F32) * f).astype(np.float64) + 0.5, top - 1).astype(np.int64)

    ix, iz = pick(hii_dim, dim), pick(hii_dim_z, dim_z)
    return np.clip(a[np.ix_(ix, ix, iz)], 0.0, 1.0)
