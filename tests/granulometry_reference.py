"""The numpy spec of the squared distance transform and the granulometry (``c21cm_granulometry_grids``,
include/c21cm_grid.h).  Everything is an integer and a function of the mask alone.

``axis_table(n, periodic)[i, j]`` is d_a(i, j)^2: |i - j| on an open axis, the minimum image min(|i - j|, n - |i - j|)
on a periodic one.  A separable transform takes, per axis, the min (or max) over j of f[j] + (or -) that table, one
axis after the other, in int64 and in slabs of lines so that the (n, n, lines) intermediate stays below 256 MiB.

``dist2(mask, periodic)``: D2[c] = min over the unselected cells q of sum_a d_a(c_a, q_a)^2; 2^30 everywhere where the
box has no unselected cell.  ``covered_mask(D2, s, periodic)``: the cells x with max_c (G[c] - |x - c|^2) > 0, G = D2
where D2 > s and minus infinity elsewhere.  ``granulometry(mask, radii2, periodic)``: every output of the C entry for
one box.  ``local_thickness`` and ``dist2_brute`` are the brute-force forms the host tests hold the transforms against.
"""

import numpy as np

NONE = 2**30
BIG = 2**40  # plus / minus infinity of the int64 transforms: above every sum of real terms
SLAB_BYTES = 256 * 2**20


def periodic3(periodic):
    return (bool(periodic),) * 3 if np.ndim(periodic) == 0 else tuple(bool(p) for p in periodic)


def axis_table(n, periodic):
    i = np.arange(n, dtype=np.int64)
    d = np.abs(i[:, None] - i[None, :])
    if periodic:
        d = np.minimum(d, n - d)
    return d * d


def transform(f, axis, periodic, sign):
    """h[i] = min_j (f[j] + d^2) for sign = +1, max_j (f[j] - d^2) for sign = -1, along ``axis``"""
    n = f.shape[axis]
    lines = np.moveaxis(f, axis, 0).reshape(n, -1).astype(np.int64)
    table = axis_table(n, periodic)[:, :, None] * sign
    out = np.empty_like(lines)
    step = max(1, SLAB_BYTES // (8 * n * n))
    for lo in range(0, lines.shape[1], step):
        t = lines[None, :, lo:lo + step] + table
        out[:, lo:lo + step] = t.min(1) if sign > 0 else t.max(1)
    moved = np.moveaxis(f, axis, 0).shape
    return np.moveaxis(out.reshape(moved), 0, axis)


def select_mask(field, threshold, below):
    v = np.asarray(field, np.float32).astype(np.float64)
    return v < threshold if below else v >= threshold


def dist2(mask, periodic=True):
    mask = np.asarray(mask, bool)
    per = periodic3(periodic)
    f = np.where(mask, BIG, 0).astype(np.int64)
    for ax in (2, 1, 0):
        f = transform(f, ax, per[ax], +1)
    return np.where(f >= BIG, NONE, f).astype(np.int32)


def covered_mask(d2, s, periodic=True):
    per = periodic3(periodic)
    g = np.where(d2 > s, d2.astype(np.int64), -BIG)
    for ax in (2, 1, 0):
        g = transform(g, ax, per[ax], -1)
    return g > 0


def granulometry(mask, radii2, periodic=True):
    """dict(covered, eroded, stats, dist2, level) of one box, as the C entry defines them"""
    mask = np.asarray(mask, bool)
    d2 = dist2(mask, periodic)
    radii2 = [int(s) for s in radii2]
    level = np.where(mask, 0, -1).astype(np.int32)
    covered, eroded = [], []
    for s in radii2:
        cov = covered_mask(d2, s, periodic) if s < int(d2.max()) else np.zeros(mask.shape, bool)
        assert not np.any(cov & ~mask)
        covered.append(int(cov.sum()))
        eroded.append(int((d2 > s).sum()))
        level += cov
    n_sel = int(mask.sum())
    flat = d2.ravel()
    deepest = int(flat.max()) if n_sel else 0
    stats = [n_sel, deepest, int(np.argmax(flat)) if n_sel else -1, mask.size - n_sel]
    return dict(covered=np.array(covered, np.int64), eroded=np.array(eroded, np.int64),
                stats=np.array(stats, np.int64), dist2=d2, level=level)


def dist2_brute(mask, periodic=True):
    """D2 from the definition: every cell against every unselected cell"""
    mask = np.asarray(mask, bool)
    per = periodic3(periodic)
    tx, ty, tz = (axis_table(n, p) for n, p in zip(mask.shape, per))
    out = np.full(mask.shape, NONE, np.int64)
    for q in np.argwhere(~mask):
        d = tx[:, q[0]][:, None, None] + ty[:, q[1]][None, :, None] + tz[:, q[2]][None, None, :]
        np.minimum(out, d, out=out)
    return out.astype(np.int32)


def local_thickness(d2, periodic=True):
    """T2[x] = the largest D2[c] over the centres c with |x - c|^2 < D2[c] (Hildebrand & Ruegsegger), 0 where there is
    none: the cell is covered at s iff T2[x] > s"""
    per = periodic3(periodic)
    tx, ty, tz = (axis_table(n, p) for n, p in zip(d2.shape, per))
    out = np.zeros(d2.shape, np.int64)
    for c in np.argwhere(d2 > 0):
        v = int(d2[tuple(c)])
        d = tx[:, c[0]][:, None, None] + ty[:, c[1]][None, :, None] + tz[:, c[2]][None, None, :]
        np.maximum(out, np.where(d < v, v, 0), out=out)
    return out


def ball_mask(shape, n_balls, seed, r_min=1.0, r_max=6.5, periodic=True):
    """the union of ``n_balls`` balls of radius r_min..r_max at random centres"""
    rng = np.random.default_rng(seed)
    per = periodic3(periodic)
    mask = np.zeros(shape, bool)
    for _ in range(n_balls):
        c = [int(rng.integers(n)) for n in shape]
        r = float(rng.uniform(r_min, r_max))
        tx, ty, tz = (axis_table(n, p) for n, p in zip(shape, per))
        d = tx[:, c[0]][:, None, None] + ty[:, c[1]][None, :, None] + tz[:, c[2]][None, None, :]
        mask |= d <= r * r
    return mask
