"""A numpy restatement of the mean-free-path bubble size estimator (c21cm_bubble_sizes_grids, include/c21cm_grid.h;
DESIGN section 4.11): the spec the device kernels are held to, ray for ray.  Everything is fp64 ``+ - * /``, ``sqrt``
and one ``cos`` / ``sin`` per ray; the rays are vectorised, the walk loops over steps with the live rays as arrays.
"""

import math

import numpy as np

from halo_sampler_reference import philox, uniform_pair

ENDED, CAPPED, ESCAPED, NO_CELL = 0, 1, 2, 255


def select_mask(box, threshold=0.5, select="below"):
    v = np.asarray(box).astype(np.float64)
    if not np.all(np.isfinite(v)):
        raise FloatingPointError("a field value is not finite")
    return v < threshold if select == "below" else v >= threshold


def draws(n_rays, seed, box_index=0):
    """(u_cell, u_x, u_y, u_z, u_mu, u_phi) of rays 0 .. n_rays - 1 of box ``box_index``"""
    r = np.arange(n_rays, dtype=np.uint64)
    out = []
    for p in range(3):
        out.extend(uniform_pair(philox(r, p, box_index, 0, int(seed))))
    return out


def max_steps(max_length, cell):
    return sum(math.ceil(max_length / c) for c in cell) + 3


def trace(mask, lengths, n_rays, seed=0, *, box_index=0, max_length=None, directions="isotropic",
          periodic=(True, True, True)):
    """The rays of one box.  ``mask``: bool (nx, ny, nz), True = selected; ``lengths``: (Lx, Ly, Lz).  Returns a dict
    of per-ray arrays: ``lengths`` (t; max_length where capped), ``flags``, ``starts`` (flat C index of the start
    cell), and ``p0`` (n, 3), ``d`` (n, 3) for checks that want the geometry.  Without a selected cell: NaN / 255 /
    -1."""
    mask = np.asarray(mask, bool)
    shape = mask.shape
    cell = [float(L) / n for L, n in zip(lengths, shape)]
    max_length = float(max(lengths)) if max_length is None else float(max_length)
    sel = np.flatnonzero(mask)
    n_sel = sel.size
    if n_sel == 0:
        return dict(lengths=np.full(n_rays, np.nan), flags=np.full(n_rays, NO_CELL, np.uint8),
                    starts=np.full(n_rays, -1, np.int64), p0=np.full((n_rays, 3), np.nan),
                    d=np.full((n_rays, 3), np.nan), n_sel=0)
    u_cell, ux, uy, uz, u_mu, u_phi = draws(n_rays, seed, box_index)
    k = np.minimum((u_cell * float(n_sel)).astype(np.int64), n_sel - 1)
    starts = sel[k].astype(np.int64)
    idx = np.stack(np.unravel_index(starts, shape), axis=1).astype(np.int64)
    u = np.stack([ux, uy, uz], axis=1)
    cellv = np.array(cell)
    p0 = (idx.astype(np.float64) + u) * cellv
    if directions == "isotropic":
        c = 2.0 * u_mu - 1.0
        s = np.sqrt(1.0 - c * c)
        phi = 2.0 * np.pi * u_phi
        d = np.stack([s * np.cos(phi), s * np.sin(phi), c], axis=1)
    elif directions == "los":
        d = np.zeros((n_rays, 3))
        d[:, 2] = np.where(u_mu >= 0.5, 1.0, -1.0)
    else:
        raise ValueError(directions)
    pos = d > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        tmax = ((idx + pos).astype(np.float64) * cellv - p0) / d
        tdel = cellv / np.abs(d)
    tmax[d == 0] = np.inf
    tdel[d == 0] = np.inf
    step = np.where(pos, 1, -1).astype(np.int64)

    out_len = np.full(n_rays, max_length)
    flags = np.full(n_rays, CAPPED, np.uint8)  # a ray that uses up its steps counts as capped
    live = np.arange(n_rays)
    n_axis = np.array(shape, np.int64)
    per = np.array(periodic, bool)
    for _ in range(max_steps(max_length, cell)):
        if live.size == 0:
            break
        tm = tmax[live]
        a = np.zeros(live.size, np.int64)
        rows = np.arange(live.size)
        a[tm[:, 1] < tm[rows, a]] = 1
        a[tm[:, 2] < tm[rows, a]] = 2
        t = tm[rows, a]
        go = t < max_length  # the others stay capped
        live, a, t = live[go], a[go], t[go]
        v = idx[live, a] + step[live, a]
        outside = (v < 0) | (v >= n_axis[a])
        esc = outside & ~per[a]
        flags[live[esc]] = ESCAPED
        out_len[live[esc]] = t[esc]
        v = np.where(v < 0, n_axis[a] - 1, np.where(v >= n_axis[a], 0, v))
        keep = ~esc
        live, a, t, v = live[keep], a[keep], t[keep], v[keep]
        idx[live, a] = v
        inside = mask[idx[live, 0], idx[live, 1], idx[live, 2]]
        end = ~inside
        flags[live[end]] = ENDED
        out_len[live[end]] = t[end]
        live, a, t = live[inside], a[inside], t[inside]
        tmax[live, a] = t + tdel[live, a]
    return dict(lengths=out_len, flags=flags, starts=starts, p0=p0, d=d, n_sel=n_sel)


def histogram(lengths, flags, edges):
    """int64 counts of the ended rays per half-open bin, as ``np.digitize(t, edges) - 1``"""
    edges = np.asarray(edges, np.float64)
    t = np.asarray(lengths)[np.asarray(flags) == ENDED]
    b = np.digitize(t, edges) - 1
    b = b[(b >= 0) & (b < edges.size - 1)]
    return np.bincount(b, minlength=edges.size - 1).astype(np.int64)


def stats(res):
    f = res["flags"]
    return np.array([res["n_sel"], np.sum(f == ENDED), np.sum(f == CAPPED), np.sum(f == ESCAPED)], np.int64)


def aabb_exit(p0, d, lo, hi):
    """The distance at which the ray p0 + t d leaves the box [lo, hi] it starts in: min over the axes of ((hi or lo)
    - p0) / d -- independent of any traversal"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (np.where(d > 0, hi, lo) - p0) / d
    t[d == 0] = np.inf
    return t.min(axis=1)


# ---- the analytic cases the host and the device tests share (the device makes the same draws) ----
CUBOID_SHAPE, CUBOID_CELL, CUBOID_BLOCK = (12, 10, 14), (1.5, 2.0, 0.75), ((3, 9), (2, 7), (5, 11))
CUBOID_SEED, CUBOID_RAYS = 7, 20000
SLAB_SHAPE, SLAB_Z, SLAB_MAX, SLAB_SEED, SLAB_RAYS = (8, 8, 16), (4, 9), 40.0, 2007, 200000
SLAB_LS = (1.0, 2.5, 5.0, 10.0, 20.0)


def cuboid_mask():
    m = np.zeros(CUBOID_SHAPE, bool)
    (a0, a1), (b0, b1), (c0, c1) = CUBOID_BLOCK
    m[a0:a1, b0:b1, c0:c1] = True
    return m


def cuboid_lengths():
    return tuple(n * c for n, c in zip(CUBOID_SHAPE, CUBOID_CELL))


def slab_mask():
    m = np.zeros(SLAB_SHAPE, bool)
    m[:, :, SLAB_Z[0]:SLAB_Z[1]] = True
    return m


def slab_survival(l, w):
    return 1.0 - l / (2.0 * w) if l <= w else w / (2.0 * l)


def check_slab(lengths, flags, w, max_length, n):
    """|p_hat - p| <= 5 sqrt(p (1 - p) / n) at every l of SLAB_LS and at the cap; returns the deviations in sigma"""
    ended = flags == ENDED
    assert np.all(ended | (flags == CAPPED))
    sig = []
    for l in SLAB_LS + (max_length,):
        p = slab_survival(l, w)
        # a capped ray is longer than every l; at l = max_length only the capped ones are
        p_hat = (np.sum(ended & (lengths > l)) + np.sum(~ended)) / n
        s = np.sqrt(p * (1.0 - p) / n)
        sig.append((p_hat - p) / s)
        assert abs(p_hat - p) <= 5.0 * s, (l, p_hat, p, s)
    return sig


def check_cuboid(res, rtol=1e-12):
    cell = np.array(CUBOID_CELL)
    lo = np.array([b[0] for b in CUBOID_BLOCK]) * cell
    hi = np.array([b[1] for b in CUBOID_BLOCK]) * cell
    want = aabb_exit(res["p0"], res["d"], lo, hi)
    assert np.all(res["flags"] == ENDED)
    rel = np.abs(res["lengths"] - want) / want
    assert rel.max() <= rtol, rel.max()
    return rel.max()
